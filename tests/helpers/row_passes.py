"""The DiT row passes of csrc/elementwise.hip (q/k RMSNorm + split RoPE, adaLN norm + modulation) as one sha256 per output buffer.
tests/test_row_passes_digests_gpu.py compares them with tests/golden/row_passes_digests.json, which
tests/golden/make_golden.py --row-passes-digests records. Every instantiation of the two kernel families is launched by at least one
case, at the smallest shapes at which it can go wrong; COVERS names the instantiation behind every group of keys and KERNELS is the
full list (the launchers' selection rules restated: np_of, nv_of):

  qk128     qknorm_rope_kernel<128, NP, XB> through ltx_op_qknorm_rope_pair: D = 1024 (NP 1), 1536 (NP 1, threads past D / 8 idle),
            2176 = 17 x 128 (NP 2, partial second chunk), 4096 at 5 rows (NP 2, below the 512-row switch), 8192 (NP 4); f32 and bf16
            rows, one and two jobs (ldx = 2 D), tables at T = 3 (row % T wraps) and none, out_scale0 = 1 and the DiT's prescale
  qk64      qknorm_rope_kernel<64, NP, false> through ltx_op_qknorm_rope_hd: D = 512, 2048, 2112 = 33 x 64, 8192 at 5 rows, T = 3
  attn64    qknorm_rope_kernel<64, NP, true>: only a bf16 context of the head-dim-64 attention module reaches it, so the digest is of
            ltx_attn_module_forward_dev's output on a synthetic module of 4, 40 and 128 heads (inner 256, 2560, 8192), a cross call
            with a bf16 context and a self-attention call
  full      D = 4096, 513 rows, T = 171 (odd row count: the last workgroup clamps its second row and breaks):
            qknorm_rope_pair_kernel<2, XB> (two jobs with tables), qknorm_rope_rows_kernel<2, XB> (one job, no tables, prescale; two
            jobs under option qknorm_no_pair = 1)
  norm      norm_mod_kernel<NV>: D = 1024, 1028, 2048, 3072, 4096, 8192 at 7 rows; RMS and LayerNorm, null scale / shift,
            round_norm_bf16, a row map, mod_bstride = 3 D with rows_per_batch = 3
  normrows  norm_mod_rows_kernel<4, 2> (515 rows, 258 per batch element) and <4, 4> (option norm_rows = 4, 517 rows, 172 per element)
  norm2     norm_mod2_kernel<NV>: (Dv, Da) = (4096, 2048) at (5, 3) rows; (1024, 8192): NV 8 fetches behind the barrier; (2048, 1028) with
            a null (scale1, shift1) pair; (1024, empty job)

Inputs are torch CPU tensors from torch.Generator().manual_seed(...) copied to the device; a digest covers the whole output buffer with
its sentinel columns and guard rows (attn64: the module's f32 output). Nothing here says that two cases give the same bits."""
import hashlib

import numpy as np
import torch

SEED = 53
EPS = 1e-6
SENTINEL = -1024.0   # exactly representable in bf16
Q_PRESCALE = float(np.float32(0.08838834764831845) * np.float32(1.4426950408889634))   # kAttnQueryPrescale (csrc/attention.h)
Q_PRESCALE64 = float(np.float32(0.125) * np.float32(1.4426950408889634))               # kAttnQueryPrescale64

QK128_SHAPES = [(1024, 5), (1536, 5), (2176, 5), (4096, 5), (8192, 3)]   # D, rows
QK64_SHAPES = [(512, 5), (2048, 5), (2112, 5), (8192, 5)]
ATTN64_HEADS = [4, 40, 128]
FULL = (4096, 513, 171)                                                   # D, rows, T
NORM_SHAPES = [(1024, 7), (1028, 7), (2048, 7), (3072, 7), (4096, 7), (8192, 7)]
NORM_VARIANTS = ["rms", "rms.round", "layer", "rms.plain", "layer.plain", "rms.rowmap"]
NORM_ROW_MAP = [2, 0, 1, 1, 0, 2, 0]
NORMROWS_CASES = [(2, 515, 258, None), (4, 517, 172, 4)]                  # R, rows, rows per batch element, option norm_rows
NORM2_CASES = [("4096x5.2048x3", (4096, 5, True), (2048, 3, True)), ("1024x5.8192x3", (1024, 5, True), (8192, 3, True)),
               ("2048x4.1028x3.null1", (2048, 4, False), (1028, 3, False)), ("1024x5.empty", (1024, 5, True), None)]


def np_of(D):
    """pair chunks per thread of the generic q/k kernel (launch_qknorm_rope)"""
    return 1 if D <= 2048 else 2 if D <= 4096 else 4


def nv_of(D):
    """float4 chunks per thread of norm_mod_kernel / norm_mod2_kernel"""
    return 1 if D <= 1024 else 2 if D <= 2048 else 4 if D <= 4096 else 8


def _b(v):
    return "true" if v else "false"


KERNELS = sorted([f"qknorm_rope_kernel<{hd}, {n}, {_b(xb)}>" for hd in (64, 128) for n in (1, 2, 4) for xb in (False, True)]
                 + [f"qknorm_rope_rows_kernel<2, {_b(xb)}>" for xb in (False, True)]
                 + [f"qknorm_rope_pair_kernel<2, {_b(xb)}>" for xb in (False, True)]
                 + [f"norm_mod_kernel<{n}>" for n in (1, 2, 4, 8)] + ["norm_mod_rows_kernel<4, 2>", "norm_mod_rows_kernel<4, 4>"]
                 + [f"norm_mod2_kernel<{n}>" for n in (1, 2, 4, 8)])


def sha(t):
    """sha256 of a device tensor's bytes, sentinel columns and guard rows included"""
    return hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def _gen(*key):
    seed = SEED
    for k in key:
        seed = seed * 1000003 + int(k)
    return torch.Generator().manual_seed(seed % (1 << 62))


def _randn(g, *shape):
    return torch.randn(shape, generator=g)


def _tables(g, T, half):
    ang = torch.rand((T, half), generator=g) * (2 * np.pi)
    return torch.cos(ang).cuda(), torch.sin(ang).cuda()


def _out(rows, ld):
    return torch.full((rows + 2, ld), SENTINEL, dtype=torch.bfloat16, device="cuda")


# ---- q/k norm + RoPE ----
def _qk_pair_variants(ctx, name, D, rows, T, group, variants):
    """variants: (x_bf16, jobs, tables, prescale); the fused q|k projection output [rows][2 D], k = the row's second half"""
    g = _gen(group, D, rows)
    qk32 = _randn(g, rows, 2 * D)
    w = (1 + 0.1 * _randn(g, 2, D)).cuda()
    cos, sin = _tables(g, T, D // 2)
    d = {}
    for xb, jobs, tables, prescale in variants:
        qk = qk32.to(torch.bfloat16).cuda() if xb else qk32.cuda()
        obuf = _out(rows, 2 * D + 8)
        c, s = (cos, sin) if tables else (None, None)
        x1, w1, o1 = (qk[:, D:], w[1], obuf[:, D:2 * D]) if jobs == 2 else (None, None, None)
        ctx.op_qknorm_rope_pair(qk[:, :D], w[0], obuf[:, :D], x1, w1, o1, c, s, T, rows, D, eps=EPS, out_scale0=Q_PRESCALE if prescale else 1.0)
        torch.cuda.synchronize()
        d[f"{name}.D{D}.{'bf16' if xb else 'f32'}.jobs{jobs}.{'rope' if tables else 'plain'}.{'prescale' if prescale else 'scale1'}"] = sha(obuf)
    return d


ALL_QK_VARIANTS = [(xb, jobs, tables, prescale) for xb in (False, True) for jobs in (1, 2) for tables in (True, False) for prescale in (False, True)]


def qk128_cases(ctx):
    d = {}
    for D, rows in QK128_SHAPES:
        d.update(_qk_pair_variants(ctx, "qk128", D, rows, 3, 1, ALL_QK_VARIANTS))
    return d


def qk64_cases(ctx):
    d = {}
    for D, rows in QK64_SHAPES:
        g = _gen(2, D, rows)
        x = _randn(g, rows, D).cuda()   # the Python wrapper takes contiguous rows
        w = (1 + 0.1 * _randn(g, D)).cuda()
        cos, sin = _tables(g, 3, D // 2)
        for tables in (True, False):
            for prescale in (False, True):
                obuf = torch.full((rows + 2, D), SENTINEL, dtype=torch.bfloat16, device="cuda")   # the op's output rows are D wide
                c, s = (cos, sin) if tables else (None, None)
                ctx.op_qknorm_rope_hd(x, w, c, s, 3, obuf[:rows], 64, out_scale=Q_PRESCALE64 if prescale else 1.0, eps=EPS)
                torch.cuda.synchronize()
                d[f"qk64.D{D}.{'rope' if tables else 'plain'}.{'prescale' if prescale else 'scale1'}"] = sha(obuf)
    return d


ATTN64_DIM, ATTN64_TQ, ATTN64_TK = 256, 5, 7


def attn64_cases(ctx):
    """the head-dim-64 module: q rows f32 (XB false), k rows bf16 behind a bf16 context (XB true); index 3 is loaded and unloaded here"""
    d = {}
    for heads in ATTN64_HEADS:
        g = _gen(3, heads)
        x = _randn(g, 1, ATTN64_TQ, ATTN64_DIM).cuda()
        context = _randn(g, 1, ATTN64_TK, ATTN64_DIM).to(torch.bfloat16).cuda()
        qt = _tables(g, ATTN64_TQ, heads * 32)
        kt = _tables(g, ATTN64_TK, heads * 32)
        ctx.attn_module_init_synthetic(3, ATTN64_DIM, ATTN64_DIM, heads, seed=SEED + heads)
        try:
            for name, c, k_tables in (("cross_bf16", context, kt), ("self", None, None)):
                out = torch.full((1, ATTN64_TQ, ATTN64_DIM), SENTINEL, dtype=torch.float32, device="cuda")
                ctx.attn_module_forward_dev(3, x, out, c, qt, k_tables)
                torch.cuda.synchronize()
                d[f"attn64.heads{heads}.{name}"] = sha(out)
        finally:
            ctx.attn_module_unload(3)
    return d


def full_width_cases(ltx, ctx):
    D, rows, T = FULL
    d = _qk_pair_variants(ctx, "full.pair", D, rows, T, 4, [(False, 2, True, True), (True, 2, True, True)])
    d.update(_qk_pair_variants(ctx, "full.rows", D, rows, T, 4, [(False, 1, False, True), (True, 1, False, True)]))
    old = ltx.get_option("qknorm_no_pair")
    ltx.set_option("qknorm_no_pair", 1)
    try:
        d.update(_qk_pair_variants(ctx, "full.rows.qknorm_no_pair=1", D, rows, T, 4, [(False, 2, True, True), (True, 2, True, True)]))
    finally:
        ltx.set_option("qknorm_no_pair", old)
    return d


# ---- norm + modulation ----
def _norm_inputs(g, rows, D, groups):
    """x as a [rows][D] view of a wider buffer; the modulation table [groups][3][D] with shift = [:, 0], scale = [:, 1] (stride 3 D)"""
    xbuf = (_randn(g, rows, D + 8) * 3 + 0.5).cuda()
    mods = (0.1 * _randn(g, groups, 3, D)).cuda()
    return xbuf, mods


def norm_cases(ctx):
    d = {}
    row_map = torch.tensor(NORM_ROW_MAP, dtype=torch.int32).cuda()
    for D, rows in NORM_SHAPES:
        xbuf, mods = _norm_inputs(_gen(5, D, rows), rows, D, 3)
        for v in NORM_VARIANTS:
            plain = v.endswith(".plain")
            obuf = _out(rows, D + 4)
            ctx.op_norm_mod_ex(xbuf[:, :D], None if plain else mods[0, 1], None if plain else mods[0, 0], obuf[:, :D], rows, D,
                               mod_bstride=mods.stride(0), rows_per_batch=3, row_map=row_map if v.endswith(".rowmap") else None,
                               norm_kind=1 if v.startswith("layer") else 0, eps=EPS, round_norm_bf16=v.endswith(".round"))
            torch.cuda.synchronize()
            d[f"norm.D{D}.{v}"] = sha(obuf)
    return d


def normrows_cases(ltx, ctx):
    d = {}
    D = 4096
    for R, rows, rpb, opt in NORMROWS_CASES:
        xbuf, mods = _norm_inputs(_gen(6, R, rows), rows, D, (rows + rpb - 1) // rpb)
        old = ltx.get_option("norm_rows")
        if opt is not None:
            ltx.set_option("norm_rows", opt)
        try:
            for rnd in (False, True):
                obuf = _out(rows, D + 4)
                ctx.op_norm_mod_ex(xbuf[:, :D], mods[0, 1], mods[0, 0], obuf[:, :D], rows, D, mod_bstride=mods.stride(0), rows_per_batch=rpb,
                                   eps=EPS, round_norm_bf16=rnd)
                torch.cuda.synchronize()
                d[f"normrows.R{R}.rows{rows}.{'round' if rnd else 'plain'}"] = sha(obuf)
        finally:
            ltx.set_option("norm_rows", old)
    return d


def norm2_cases(ctx):
    d = {}
    for name, video, audio in NORM2_CASES:
        jobs, outs = [], []
        for i, spec in enumerate((video, audio)):
            if spec is None:
                jobs.append(None)
                continue
            D, rows, both = spec
            xbuf, mods = _norm_inputs(_gen(7, i, D, rows), rows, D, 2)   # [2][3][D] is read as four vectors of one modulation row
            o0, o1 = _out(rows, D + 4), _out(rows, D + 4)
            outs += [o0, o1]
            jobs.append(dict(x=xbuf[:, :D], out0=o0[:, :D], out1=o1[:, :D], rows=rows, D=D, scale0=mods[0, 1], shift0=mods[0, 0],
                             scale1=mods[1, 1] if both else None, shift1=mods[1, 0] if both else None, mod_bstride=0, rows_per_batch=rows))
        ctx.op_norm_mod2(jobs[0], jobs[1], eps=EPS)
        torch.cuda.synchronize()
        for i, o in enumerate(outs):
            d[f"norm2.{name}.{'va'[i // 2]}.out{i % 2}"] = sha(o)
    return d


def all_cases(ltx, ctx):
    d = {}
    for part in (qk128_cases(ctx), qk64_cases(ctx), attn64_cases(ctx), full_width_cases(ltx, ctx), norm_cases(ctx), normrows_cases(ltx, ctx),
                 norm2_cases(ctx)):
        assert not set(d) & set(part)
        d.update(part)
    return d


def _qk_keys(name, D, variants):
    return [f"{name}.D{D}.{'bf16' if xb else 'f32'}.jobs{jobs}.{'rope' if t else 'plain'}.{'prescale' if p else 'scale1'}" for xb, jobs, t, p in variants]


def covers():
    """key -> the instantiation whose output the digest is (attn64: the two q/k launches of the module forward)"""
    c = {}
    for D, _ in QK128_SHAPES:
        for k, v in zip(_qk_keys("qk128", D, ALL_QK_VARIANTS), ALL_QK_VARIANTS):
            c[k] = [f"qknorm_rope_kernel<128, {np_of(D)}, {_b(v[0])}>"]
    for D, _ in QK64_SHAPES:
        for t in ("rope", "plain"):
            for p in ("scale1", "prescale"):
                c[f"qk64.D{D}.{t}.{p}"] = [f"qknorm_rope_kernel<64, {np_of(D)}, false>"]
    for heads in ATTN64_HEADS:
        n = np_of(heads * 64)
        c[f"attn64.heads{heads}.cross_bf16"] = [f"qknorm_rope_kernel<64, {n}, false>", f"qknorm_rope_kernel<64, {n}, true>"]
        c[f"attn64.heads{heads}.self"] = [f"qknorm_rope_kernel<64, {n}, false>"]
    D = FULL[0]
    for xb in (False, True):
        c[_qk_keys("full.pair", D, [(xb, 2, True, True)])[0]] = [f"qknorm_rope_pair_kernel<2, {_b(xb)}>"]
        c[_qk_keys("full.rows", D, [(xb, 1, False, True)])[0]] = [f"qknorm_rope_rows_kernel<2, {_b(xb)}>"]
        c[_qk_keys("full.rows.qknorm_no_pair=1", D, [(xb, 2, True, True)])[0]] = [f"qknorm_rope_rows_kernel<2, {_b(xb)}>"]
    for D, _ in NORM_SHAPES:
        for v in NORM_VARIANTS:
            c[f"norm.D{D}.{v}"] = [f"norm_mod_kernel<{nv_of(D)}>"]
    for R, rows, _, _ in NORMROWS_CASES:
        for r in ("plain", "round"):
            c[f"normrows.R{R}.rows{rows}.{r}"] = [f"norm_mod_rows_kernel<4, {R}>"]
    for name, video, audio in NORM2_CASES:
        nv = nv_of(max(s[0] for s in (video, audio) if s))
        for i, s in enumerate((video, audio)):
            if s:
                for o in (0, 1):
                    c[f"norm2.{name}.{'va'[i]}.out{o}"] = [f"norm_mod2_kernel<{nv}>"]
    return c


def expected_keys():
    return sorted(covers())
