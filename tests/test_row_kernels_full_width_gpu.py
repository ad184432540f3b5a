"""The row kernels the DiT runs at full width (D = 4096, 512 rows and more), each against a float64 restatement of its formula.

launch_norm_mod and launch_qknorm_rope (csrc/elementwise.hip) leave their generic one-row-per-workgroup kernels at D == 4096 and
rows >= 512 for norm_mod_rows_kernel<4, 2 | 4>, qknorm_rope_pair_kernel<2, f32 | bf16> and qknorm_rope_rows_kernel<2, f32 | bf16>. Whole
forwards see those at rel-L2 1e-2; here every ELEMENT is held to the rounding of its own value. The calls go through the two test
seams ltx_op_norm_mod_ex / ltx_op_qknorm_rope_pair, which pass every argument of the launchers.

Reference: float64 torch on the device, from the very values the kernel reads (bf16 inputs as their bf16 values, eps and the query
prescale as the f32 numbers the C call receives), rounded to bf16 ONCE (bf16_round64: integer arithmetic on the exponent, no detour
through f32). Never the library's generic kernel.

Bound per element: |got - ref64| <= half a bf16 ulp of ref64 + A. A is the f32-evaluation allowance for values that cancel to near
zero; it is MEASURED (allowance(), on the CPU) as the largest |r32 - ref64| over two float32 numpy restatements of the formula whose
sums of squares run in different orders (numpy's pairwise sum; 64 strided partial sums added in sequence), times a margin of 4 because
the kernel's order (16 or 32 values per lane, a butterfly over 64 lanes, four waves in order) is a third one. Measured on
1537 x 4096 rows of the tests' own distributions: norm + modulation 1.52e-6 (A = 6.1e-6), q-norm + RoPE 1.31e-6 (A = 5.2e-6; the
query's is multiplied by its prescale). In addition at most 1e-3 of the elements of a case may differ from bf16(ref64) at all: a
second rounding or a sub-ulp bias moves tens of percent, f32 against f64 evaluation moves 2e-5 to 3e-5.

round_norm_bf16 has an inner rounding point: norm(x) goes through bf16 before the modulation. Where norm64 lies within A of a bf16 tie
the f32 evaluation may legitimately round the other way; for those elements (and only those) the reference with the other neighbour
is accepted too. They count as differing elements under the 1e-3 cap.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

D = 4096
HEADS = 32
EPS = float(np.float32(1e-6))
# kAttnQueryPrescale (csrc/attention.h): (1 / sqrt(128)) * log2(e), the product of the two f32 constants
Q_PRESCALE = float(np.float32(0.08838834764831845) * np.float32(1.4426950408889634))
SENTINEL = -1024.0   # exactly representable in bf16
MAX_DIFFERING = 1e-3
MARGIN = 4.0


# ---------------------------------------------------------------------------------------------------------------
# float64 helpers (device or host tensors)
# ---------------------------------------------------------------------------------------------------------------
def _exponent(v):
    """floor(log2 |v|) of a float64 tensor from its exponent bits (zeros and subnormals: clamped far below any bf16 of interest)"""
    return (((v.contiguous().view(torch.int64) >> 52) & 0x7FF) - 1023).clamp(min=-200)


def _exp2(k):
    return ((k + 1023) << 52).view(torch.float64)


def bf16_round64(v):
    """nearest bf16 value of a float64 tensor, ties to even, as float64: one rounding"""
    q = _exp2(_exponent(v) - 7)          # one bf16 ulp in v's binade
    return torch.round(v / q) * q        # the quotient and the product are exact (powers of two); torch.round is half-to-even


def half_ulp(v):
    return torch.where(v == 0, torch.zeros_like(v), _exp2(_exponent(v) - 8))


def test_bf16_round64_matches_the_f32_rounding_rule():
    """the helper against torch's own f32 -> bf16 conversion on f32 values (where no double rounding can occur), ties included"""
    g = torch.Generator().manual_seed(0)
    v = torch.randn(1 << 16, generator=g) * 3
    v = torch.cat([v, torch.tensor([0.0, 1.0, -1.0, 1.00390625, 1.01171875, 255.5, 0.99609375, 3.0e-5, -6.5])])
    assert torch.equal(bf16_round64(v.double()), v.to(torch.bfloat16).double())
    assert float(half_ulp(torch.tensor([1.5], dtype=torch.float64))) == 2.0 ** -8


def check(got_bf16, ref64, A, what, alt64=None, alt_ok=None):
    """the per-element bound and the share of elements that differ from bf16(ref64); prints both figures before it asserts"""
    got = got_bf16.double()
    assert bool(torch.isfinite(got).all()), what
    err = (got - ref64).abs()
    ok = err <= half_ulp(ref64) + A
    if alt64 is not None:
        ok |= alt_ok & ((got - alt64).abs() <= half_ulp(alt64) + A)
    share = float((got != bf16_round64(ref64)).double().mean())
    worst = float((err / (half_ulp(ref64) + A)).max())
    print(f"{what}: worst |got - ref64| / (half ulp + A) = {worst:.3f}, share differing from bf16(ref64) = {share:.2e}, "
          f"outside the bound: {int((~ok).sum())}")
    assert bool(ok.all()), (what, worst, int((~ok).sum()))
    assert share <= MAX_DIFFERING, (what, share)


# ---------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------
def norm_mod_ref64(x, scale, shift, mod_row, kind, eps, round_norm, A):
    """x [rows, D] (any float dtype, the values the kernel reads), scale / shift [G, D], mod_row int64 [rows]: the modulation row of each
    row. Returns (ref64, alt64, alt_ok): alt is the reference with the OTHER bf16 neighbour at round_norm_bf16's inner rounding point,
    valid where alt_ok (norm64 within A of a tie); None, None without that rounding."""
    x64 = x.double()
    if kind == 0:
        n = x64 / torch.sqrt((x64 * x64).mean(1, keepdim=True) + eps)
    else:
        d = x64 - x64.mean(1, keepdim=True)
        n = d / torch.sqrt((d * d).mean(1, keepdim=True) + eps)
    s1 = 1.0 + scale.double()[mod_row]
    h = shift.double()[mod_row]
    if not round_norm:
        return n * s1 + h, None, None
    nr = bf16_round64(n)
    ulp = 2.0 * half_ulp(n)
    other = nr + torch.where(n >= nr, ulp, -ulp)
    near_tie = (n - nr).abs() >= half_ulp(n) - A
    return nr * s1 + h, other * s1 + h, near_tie


def qknorm_rope_ref64(x, w, cos, sin, T, out_scale):
    """x [rows, D] f32 or bf16, w [D], cos / sin [T, D / 2] or None: RMSNorm over all heads * w, split RoPE per head (first half of a head
    against its second half), * out_scale."""
    rows = x.shape[0]
    x64 = x.double()
    n = x64 / torch.sqrt((x64 * x64).mean(1, keepdim=True) + EPS) * w.double()
    if cos is not None:
        t = torch.arange(rows, device=x.device) % T
        c = cos.double()[t].view(rows, HEADS, 64)
        s = sin.double()[t].view(rows, HEADS, 64)
        n = n.view(rows, HEADS, 2, 64)
        a, b = n[:, :, 0], n[:, :, 1]
        n = torch.stack([a * c - b * s, b * c + a * s], dim=2).reshape(rows, D)
    return n * out_scale


@functools.lru_cache(maxsize=None)
def allowance(family):
    """A of the module docstring, measured on the CPU (numpy float32 against float64) on 1537 rows of the tests' distributions"""
    rng = np.random.default_rng(123)
    rows = 1537

    def ms_pairwise(v):
        return (v * v).sum(1, keepdims=True, dtype=np.float32) / np.float32(D)

    def ms_strided(v):
        p = (v * v).reshape(rows, D // 64, 64)
        acc = np.zeros((rows, 64), np.float32)
        for j in range(D // 64):
            acc = acc + p[:, j]
        tot = np.zeros((rows,), np.float32)
        for j in range(64):
            tot = tot + acc[:, j]
        return (tot / np.float32(D))[:, None]

    eps = np.float32(1e-6)
    worst = 0.0
    if family == "norm_mod":
        x = (rng.standard_normal((rows, D)) * 3 + 0.5).astype(np.float32)
        sc = (0.1 * rng.standard_normal(D)).astype(np.float32)
        sh = (0.1 * rng.standard_normal(D)).astype(np.float32)
        x64 = x.astype(np.float64)
        ref = x64 / np.sqrt((x64 * x64).mean(1, keepdims=True) + float(eps)) * (1.0 + sc.astype(np.float64)) + sh
        for ms in (ms_pairwise, ms_strided):
            r32 = x * (np.float32(1) / np.sqrt(ms(x) + eps)) * (np.float32(1) + sc) + sh
            assert r32.dtype == np.float32
            worst = max(worst, float(np.abs(r32 - ref).max()))
    else:
        x = torch.from_numpy(rng.standard_normal((rows, D)).astype(np.float32)).to(torch.bfloat16).float().numpy()
        w = (1 + 0.1 * rng.standard_normal(D)).astype(np.float32)
        ang = rng.uniform(0, 2 * np.pi, (rows, D // 2))
        c, s = np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)
        ref = qknorm_rope_ref64(torch.from_numpy(x), torch.from_numpy(w), torch.from_numpy(c), torch.from_numpy(s), rows, 1.0).numpy()
        for ms in (ms_pairwise, ms_strided):
            n = (x * (np.float32(1) / np.sqrt(ms(x) + eps)) * w).reshape(rows, HEADS, 2, 64)
            a, b = n[:, :, 0], n[:, :, 1]
            c3, s3 = c.reshape(rows, HEADS, 64), s.reshape(rows, HEADS, 64)
            r32 = np.stack([a * c3 - b * s3, b * c3 + a * s3], axis=2).reshape(rows, D)
            assert r32.dtype == np.float32
            worst = max(worst, float(np.abs(r32 - ref).max()))
    print(f"allowance({family}): largest |r32 - ref64| = {worst:.3e}, A = {MARGIN * worst:.3e}")
    assert 0 < worst < 1e-5, worst   # an f32 evaluation of values of magnitude <= 8: a larger figure means the restatement is wrong
    return MARGIN * worst


# ---------------------------------------------------------------------------------------------------------------
# norm + modulation
# ---------------------------------------------------------------------------------------------------------------
def rows_kernel_expected(rows, rpb, norm_rows=0, kind=0, row_map=False):
    """launch_norm_mod's selection, restated: (takes norm_mod_rows_kernel, R)"""
    R = norm_rows if norm_rows in (2, 4) else (2 if rows <= 3072 else 4)
    return (kind == 0 and not row_map and rows >= 512 and rpb % R == 0), R


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def make_norm_inputs(rows, groups, seed, ldx=D + 8, x_std=3.0, x_mean=0.5, mod_rows=3):
    """x as a [rows, D] view of a wider buffer with NaN sentinel columns and two NaN guard rows (a kernel that reads them poisons its
    sum); the modulation table [groups, mod_rows, D] with shift = [:, 0], scale = [:, 1] (the order dit.cpp passes)"""
    g = _gen(seed)
    xbuf = torch.full((rows + 2, ldx), float("nan"), device="cuda")
    xbuf[:rows, :D] = torch.randn((rows, D), generator=g, device="cuda") * x_std + x_mean
    mods = 0.1 * torch.randn((groups, mod_rows, D), generator=g, device="cuda")
    return xbuf, mods


def run_norm_mod(ctx, xbuf, mods, rows, rpb, ldo=D + 4, row_map=None, kind=0, round_norm=False):
    obuf = torch.full((rows + 2, ldo), SENTINEL, device="cuda", dtype=torch.bfloat16)
    ctx.op_norm_mod_ex(xbuf[:, :D], mods[0, 1], mods[0, 0], obuf[:, :D], rows, D, mod_bstride=mods.stride(0), rows_per_batch=rpb,
                       row_map=row_map, norm_kind=kind, eps=EPS, round_norm_bf16=round_norm)
    torch.cuda.synchronize()
    assert bool((obuf[rows:] == SENTINEL).all()), "guard rows behind the last row were written"
    assert bool((obuf[:, D:] == SENTINEL).all()), "sentinel columns beyond D were written"
    return obuf[:rows, :D]


# rows, batch elements, and the kernel the launcher's conditions select (RMS, modulated, no row map, D == 4096, rows >= 512,
# rows_per_batch % R == 0 with R = 2 up to 3072 rows and 4 above)
NORM_ROWS_CASES = [
    (512, 1, "rows<2>"),     # the threshold itself
    (1536, 1, "rows<2>"),
    (3072, 1, "rows<2>"),    # the last launch with two rows per workgroup
    (3076, 1, "rows<4>"),    # 3076 % 4 == 0: stays on the rows kernel
    (6144, 1, "rows<4>"),
    (9984, 1, "rows<4>"),
    (1536, 2, "rows<2>"),    # 2 x 768, a modulation row per batch element: row 768 starts element 1
    (3072, 3, "rows<2>"),    # 3 x 1024
    (3078, 3, "generic"),    # 3 x 1026 at R = 4: 1026 % 4 != 0 -> one row per workgroup
]


@pytest.mark.parametrize("round_norm", [False, True])
@pytest.mark.parametrize("rows,B,kernel", NORM_ROWS_CASES)
def test_norm_mod_rows_kernel_vs_float64(gpu_ctx, rows, B, kernel, round_norm):
    rpb = rows // B
    takes, R = rows_kernel_expected(rows, rpb)
    assert (f"rows<{R}>" if takes else "generic") == kernel and rpb * B == rows
    A = allowance("norm_mod")
    xbuf, mods = make_norm_inputs(rows, B, seed=rows + B)
    got = run_norm_mod(gpu_ctx, xbuf, mods, rows, rpb, round_norm=round_norm)
    mod_row = torch.arange(rows, device="cuda") // rpb
    ref, alt, alt_ok = norm_mod_ref64(xbuf[:rows, :D], mods[:, 1], mods[:, 0], mod_row, 0, EPS, round_norm, A)
    check(got, ref, A, f"norm_mod {kernel} rows={rows} B={B} round_norm={int(round_norm)}", alt, alt_ok)
    if B > 1:  # the cases must be able to tell the batch elements apart: the reference with element 0's row everywhere is far off
        wrong, _, _ = norm_mod_ref64(xbuf[:rows, :D], mods[:, 1], mods[:, 0], torch.zeros_like(mod_row), 0, EPS, False, A)
        assert float(((got.double() - wrong).abs() > half_ulp(wrong) + A).double().mean()) > 0.3


@pytest.mark.parametrize("rows,kernel", [(1536, "rows<2>"), (6144, "rows<4>")])
def test_norm_mod_rows_kernel_zero_row_and_tiny_rms(gpu_ctx, rows, kernel):
    """An all-zero row gives exactly the shift (0 * rsqrt(eps) stays 0, finite); rows of rms 1e-3 make eps = 1e-6 half of what stands
    under the root (mean square 1e-6), so a kernel that forgot or misplaced eps is off by 40 %."""
    takes, R = rows_kernel_expected(rows, rows)
    assert takes and f"rows<{R}>" == kernel
    A = allowance("norm_mod")
    xbuf, mods = make_norm_inputs(rows, 1, seed=7, x_std=3.0 * 1e-3 / 3.04, x_mean=0.5 * 1e-3 / 3.04)
    zero_rows = [5, rows - 1]
    xbuf[zero_rows, :D] = 0.0
    got = run_norm_mod(gpu_ctx, xbuf, mods, rows, rows)
    x = xbuf[:rows, :D]
    rms = x[0].double().pow(2).mean().sqrt()
    assert 0.5e-3 < float(rms) < 2e-3
    mod_row = torch.zeros(rows, dtype=torch.int64, device="cuda")
    ref, _, _ = norm_mod_ref64(x, mods[:, 1], mods[:, 0], mod_row, 0, EPS, False, A)
    check(got, ref, A, f"norm_mod {kernel} rows={rows} tiny rms, zero rows")
    assert torch.equal(got[zero_rows], mods[0, 0].to(torch.bfloat16).expand(2, D)), "an all-zero row must give the shift"
    no_eps, _, _ = norm_mod_ref64(x, mods[:, 1], mods[:, 0], mod_row, 0, 0.0, False, A)
    assert float((no_eps[0] - ref[0]).abs().max() / ref[0].abs().max()) > 0.1, "eps carries no weight in this case"


@pytest.mark.parametrize("round_norm", [False, True])
def test_norm_mod_rows_kernels_and_generic_kernel_give_the_same_bits(gpu_ctx, ltx, round_norm):
    """elementwise.hip says the rows kernel sums "in the same order as norm_mod_kernel's block_reduce_sum": 16 squares per lane in
    register order, the 64-lane butterfly, the four wave sums in wave order, one rsqrtf, the same multiply-add. So two rows per
    workgroup, four rows per workgroup (option `norm_rows`) and the same rows launched in slices of 384 (< 512 rows: the generic kernel)
    must agree bit for bit."""
    rows, B = 1536, 2
    rpb = rows // B
    xbuf, mods = make_norm_inputs(rows, B, seed=99)
    assert rows_kernel_expected(rows, rpb, 2) == (True, 2) and rows_kernel_expected(rows, rpb, 4) == (True, 4)
    outs = {}
    for r in (2, 4):
        with gpu_ctx.options(norm_rows=r):
            outs[r] = run_norm_mod(gpu_ctx, xbuf, mods, rows, rpb, round_norm=round_norm).clone()
    assert ltx.get_option("norm_rows") == 0
    sliced = torch.empty_like(outs[2])
    n = 384
    assert rows_kernel_expected(n, n)[0] is False and rpb % n == 0
    for r0 in range(0, rows, n):
        xs = torch.full((n + 2, xbuf.shape[1]), float("nan"), device="cuda")
        xs[:n] = xbuf[r0:r0 + n]
        b = r0 // rpb
        sliced[r0:r0 + n] = run_norm_mod(gpu_ctx, xs, mods[b:b + 1], n, n, round_norm=round_norm)
    assert torch.equal(outs[2].view(torch.int16), outs[4].view(torch.int16))
    assert torch.equal(outs[2].view(torch.int16), sliced.view(torch.int16))


def test_norm_mod_generic_kernel_with_row_map_and_layer_norm_head(gpu_ctx):
    """norm_mod_kernel<4> as image-to-video and the output head call it (dit.cpp): a row map of the kind i2v_rowmap_kernel builds,
    row_map[b * T + t] = b * G + (t < first) with G = 2 and a different modulation row for each of the B * G = 4 groups (RMS, stride
    3 D here as any table stride); LayerNorm with mod_bstride = 2 D (the head's [B][2][D] table: shift, then scale) without and with the
    map. A row map sends every launch to the generic kernel, 1400 rows notwithstanding."""
    A = allowance("norm_mod")
    B, T, G, first = 2, 700, 2, 175
    rows = B * T
    assert rows_kernel_expected(rows, T, row_map=True)[0] is False and rows_kernel_expected(rows, T, kind=1)[0] is False
    t = torch.arange(rows, device="cuda")
    row_map = ((t // T) * G + ((t % T) < first).long()).to(torch.int32)
    assert sorted(set(row_map.tolist())) == [0, 1, 2, 3] and int(row_map[0]) == 1 and int(row_map[first]) == 0 and int(row_map[T]) == 3
    xbuf, mods = make_norm_inputs(rows, B * G, seed=31)
    got = run_norm_mod(gpu_ctx, xbuf, mods, rows, T, row_map=row_map)
    x = xbuf[:rows, :D]
    ref, _, _ = norm_mod_ref64(x, mods[:, 1], mods[:, 0], row_map.long(), 0, EPS, False, A)
    check(got, ref, A, "norm_mod generic, RMS, row map")
    other = row_map.long() ^ 1   # the batch element's other group
    wrong, _, _ = norm_mod_ref64(x, mods[:, 1], mods[:, 0], other, 0, EPS, False, A)
    assert float(((got.double() - wrong).abs() > half_ulp(wrong) + A).double().mean()) > 0.3
    # the output head: LayerNorm, table [groups][2][D]
    xbuf, mods = make_norm_inputs(rows, B * G, seed=32, mod_rows=2)
    assert mods.stride(0) == 2 * D
    for rm, mod_row in ((None, t // T), (row_map, row_map.long())):
        got = run_norm_mod(gpu_ctx, xbuf, mods, rows, T, row_map=rm, kind=1)
        ref, _, _ = norm_mod_ref64(xbuf[:rows, :D], mods[:, 1], mods[:, 0], mod_row, 1, EPS, False, A)
        check(got, ref, A, f"norm_mod generic, LayerNorm, stride 2 D, row map {rm is not None}")


# ---------------------------------------------------------------------------------------------------------------
# q / k RMSNorm + RoPE
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rope_tables_dev(ltx, F, H, W):
    cfg = ltx.default_transformer_config()
    assert cfg.num_attention_heads == HEADS and cfg.num_attention_heads * cfg.attention_head_dim == D
    cos, sin = ltx.rope_tables(cfg, F, H, W)
    return torch.from_numpy(cos).cuda(), torch.from_numpy(sin).cuda()


def make_qk(rows, x_bf16, seed):
    """the fused q|k projection output [rows, 2 D] as dit.cpp holds it (ldx = 2 D, k = base + D elements of the row's type), N(0, 1),
    behind it two guard rows of NaN; norm weights 1 + 0.1 N(0, 1)"""
    g = _gen(seed)
    qk = torch.full((rows + 2, 2 * D), float("nan"), device="cuda")
    qk[:rows] = torch.randn((rows, 2 * D), generator=g, device="cuda")
    if x_bf16:
        qk = qk.to(torch.bfloat16)
    w = 1 + 0.1 * torch.randn((2, D), generator=g, device="cuda")
    return qk, w


def run_qk(ctx, qk, w, cos, sin, T, rows, jobs=2, ldo=2 * D + 8):
    """q -> columns [0, D), k -> [D, 2 D) of one output buffer with sentinel columns behind them and two guard rows"""
    obuf = torch.full((rows + 2, ldo), SENTINEL, device="cuda", dtype=torch.bfloat16)
    if jobs == 2:
        ctx.op_qknorm_rope_pair(qk[:, :D], w[0], obuf[:, :D], qk[:, D:], w[1], obuf[:, D:2 * D], cos, sin, T, rows, D, eps=EPS,
                                out_scale0=Q_PRESCALE)
    else:
        ctx.op_qknorm_rope_pair(qk[:, :D], w[0], obuf[:, :D], None, None, None, cos, sin, T, rows, D, eps=EPS, out_scale0=Q_PRESCALE)
    torch.cuda.synchronize()
    assert bool((obuf[rows:] == SENTINEL).all()), "guard rows behind the last row were written"
    assert bool((obuf[:, jobs * D:] == SENTINEL).all()), "columns beyond the jobs' outputs were written"
    return obuf[:rows, :D], obuf[:rows, D:2 * D]


def qk_kernel_expected(rows, jobs, tables, no_pair=False):
    """launch_qknorm_rope's selection at D == 4096, restated"""
    if rows >= 512 and jobs == 2 and tables and not no_pair:
        return "pair"
    return "rows" if rows >= 512 else "generic"


# (F, H, W) of the latent -> T tokens per batch element, batch elements. 585 = 5 x 9 x 13 is odd: with B = 1 the last workgroup has
# one row; with B = 2 rows 584 and 585 share a workgroup and need table rows 584 and 0.
QK_SHAPES = [((2, 16, 16), 1), ((4, 16, 24), 1), ((4, 32, 48), 1), ((5, 9, 13), 1), ((5, 9, 13), 2)]


@pytest.mark.parametrize("x_bf16", [False, True])
@pytest.mark.parametrize("kernel", ["pair", "rows"])
@pytest.mark.parametrize("fhw,B", QK_SHAPES)
def test_qknorm_rope_full_width_kernels_vs_float64(gpu_ctx, ltx, fhw, B, kernel, x_bf16):
    """qknorm_rope_pair_kernel<2, x_bf16> (q and k jobs together, tables: every self-attention; bf16 input is the default) and
    qknorm_rope_rows_kernel<2, x_bf16> (one job with tables, out_scale on it: what `qknorm_no_pair` and a lone job run)."""
    T = fhw[0] * fhw[1] * fhw[2]
    rows = B * T
    assert rows in (512, 1536, 6144, 585, 1170)
    jobs = 2 if kernel == "pair" else 1
    assert qk_kernel_expected(rows, jobs, True) == kernel
    A = allowance("qknorm_rope")
    cos, sin = rope_tables_dev(ltx, *fhw)
    qk, w = make_qk(rows, x_bf16, seed=rows + 2 * int(x_bf16))
    q, k = run_qk(gpu_ctx, qk, w, cos, sin, T, rows, jobs)
    what = f"qknorm_rope {kernel} {'bf16' if x_bf16 else 'f32'} rows={rows} T={T}"
    ref_q = qknorm_rope_ref64(qk[:rows, :D], w[0], cos, sin, T, Q_PRESCALE)
    check(q, ref_q, A * Q_PRESCALE, what + " q")
    if jobs == 2:
        check(k, qknorm_rope_ref64(qk[:rows, D:], w[1], cos, sin, T, 1.0), A, what + " k")
    if B == 2:  # the case must see the wrap of row % T inside a workgroup: row T with table row T instead of 0 is far off
        t_wrong = torch.full((1,), T - 1, device="cuda")
        wrong = qknorm_rope_ref64(qk[T:T + 1, :D], w[0], cos[t_wrong], sin[t_wrong], 1, Q_PRESCALE)
        assert float(((q[T:T + 1].double() - wrong).abs() > half_ulp(wrong) + A).double().mean()) > 0.3


@pytest.mark.parametrize("x_bf16", [False, True])
@pytest.mark.parametrize("jobs", [1, 2])
def test_qknorm_without_tables_at_full_width_vs_float64(gpu_ctx, jobs, x_bf16):
    """No RoPE tables: qknorm_rope_rows_kernel<2, x_bf16> (the pair kernel needs tables). One job with the prescale is the cross-attention
    query of every block (dit.cpp, launch_qknorm_rope with null tables). Two jobs without tables are not launched by the pipeline (the
    cross-attention k pass is a single job over the context rows, usually fewer than 512); the launcher accepts them, so they are held
    to the same bound."""
    rows = 1536
    assert qk_kernel_expected(rows, jobs, False) == "rows"
    A = allowance("qknorm_rope")
    qk, w = make_qk(rows, x_bf16, seed=17 + int(x_bf16))
    q, k = run_qk(gpu_ctx, qk, w, None, None, rows, rows, jobs)
    what = f"qknorm (no tables) rows kernel {'bf16' if x_bf16 else 'f32'} jobs={jobs}"
    check(q, qknorm_rope_ref64(qk[:rows, :D], w[0], None, None, rows, Q_PRESCALE), A * Q_PRESCALE, what + " q")
    if jobs == 2:
        check(k, qknorm_rope_ref64(qk[:rows, D:], w[1], None, None, rows, 1.0), A, what + " k")


@pytest.mark.parametrize("x_bf16", [False, True])
def test_qknorm_no_pair_option_stays_within_one_rounding_of_the_pair_kernel(gpu_ctx, ltx, x_bf16):
    """Option `qknorm_no_pair` = 1 runs q and k on qknorm_rope_rows_kernel (grid.y = 2) instead of qknorm_rope_pair_kernel. Read side by
    side the two kernels write every value with the same expressions: the sum of squares as 16 terms a * a + b * b per lane in the same
    (j, e) order, the 64-lane butterfly, the four wave sums added in wave order, one rsqrtf, then x * rstd * w, the rotation and the
    prescale. Equal bits were expected and are NOT what an MI355X gives: on this case 31 to 49 of 4.8 M elements per job differ (1e-5),
    scattered over as many rows, each kernel the closer one to float64 about half the time - the signature of a last-bit f32 difference
    (the compiler contracts a * a + b * b and a0 * c - b0 * s into fused multiply-adds per kernel, and chooses differently), not of another
    summation order. So the assertion is the one for two f32 evaluations of one formula: every element within one bf16 ulp of the
    float64 value (plus A, for rotated values that cancel to near zero), at most 1e-3 of them different at all, and the option is flagged
    `numerics` in the option table. T = 585 with B = 2 covers the last one-row workgroup and the wrap of row % T."""
    fhw, B = (5, 9, 13), 2
    T = 585
    rows = B * T
    A = allowance("qknorm_rope")
    cos, sin = rope_tables_dev(ltx, *fhw)
    qk, w = make_qk(rows, x_bf16, seed=5)
    assert qk_kernel_expected(rows, 2, True) == "pair" and qk_kernel_expected(rows, 2, True, no_pair=True) == "rows"
    q0, k0 = (t.clone() for t in run_qk(gpu_ctx, qk, w, cos, sin, T, rows))
    with gpu_ctx.options(qknorm_no_pair=1):
        q1, k1 = run_qk(gpu_ctx, qk, w, cos, sin, T, rows)
    assert ltx.get_option("qknorm_no_pair") == 0
    assert dict((t[0], t[4]) for t in ltx.option_table())["qknorm_no_pair"] is True
    for name, a, b, x, wj, sc in (("q", q0, q1, qk[:rows, :D], w[0], Q_PRESCALE), ("k", k0, k1, qk[:rows, D:], w[1], 1.0)):
        ref = qknorm_rope_ref64(x, wj, cos, sin, T, sc)
        diff = (a.double() - b.double()).abs()
        share = float((diff != 0).double().mean())
        worst = float((diff / (2 * half_ulp(ref) + A * sc)).max())
        print(f"pair against rows kernel, {'bf16' if x_bf16 else 'f32'} {name}: share of differing elements {share:.2e}, worst / (ulp + A) {worst:.3f}")
        assert bool((diff <= 2 * half_ulp(ref) + A * sc).all()) and share <= MAX_DIFFERING, (name, share, worst)
