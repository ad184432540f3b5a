"""The branches of launch_gemm_bf16 (csrc/gemm.hip) that launch more than one kernel or pick a split count, as one sha256 per output
buffer. tests/test_gemm_launcher_paths_gpu.py compares them with tests/golden/gemm_launcher_paths_digests.json, which
tests/golden/make_golden.py --gemm-launcher-paths-digests records. The rules below are the launcher's for 256 CUs; the shapes are the
smallest that reach each branch (kernel names of a recording run, profiles/launcher_refactor_trace.txt):

  rowsplit  dense 6336 x 4096 x 128: 33 x 16 = 528 tiles of 192 x 256 = two rounds + 16 -> a head of 32 row tiles on that kernel and a tail
            of one row tile through the tile choice again; and with option gemm_rowsplit = 0 (one launch)
  fewrow    128 x 1024 x 2048 with a workspace and the split left to the launcher: 128 x 64 ring tiles (cfg 29), four K ranges, finish
            pass, then the norm pass as its own launch
  dtl_split 1536 x 4096 x 16384, the same seam: two K ranges of the 192 x 256 kernel with the fused finish + norm pass; and with option
            finish_norm = 0 (plain finish pass + norm pass)
  conv tail 64 -> 128 channels at 5 x 416 x 48: 520 tiles of 192 x 128 = the halo-staged kernel on 512 + a three-way split-K window of 8 on
            the ring kernel; and with option conv_no_tail = 1 (one launch)
  conv tall 64 -> 128 channels at 5 x 128 x 192: 320 tiles of 384 x 128 = one round of 256 + 64 as 128 tiles of 192 x 128 behind it; with
            conv_tall = 0 (192-row tiles and their own tail) and with conv_halo = 0 (ring kernel)
  conv narrow  64 -> 48 channels at 2 x 16 x 48: cfg 27, the 192 x 64 instance of the halo-staged kernel

Inputs come from numpy.random.default_rng([SEED, ...shape]) (uniform, so that every sum rounds: the order of a reduction shows); a digest
covers the whole output buffer with its poisoned border. Nothing here says that two option values give the same bits - each digest is
its own record."""
import contextlib
import hashlib

import numpy as np
import torch

SEED = 31
POISON = -777.0
NCU = 256                                  # the CU count the shapes were worked out for
ROWSPLIT_SHAPE = (6336, 4096, 128)         # M, N, K
FEWROW_SHAPE = (128, 1024, 2048)
DTL_SPLIT_SHAPE = (1536, 4096, 16384)
CONV_TAIL = (5, 416, 48, 64, 128)          # F, H, W, Cin, Cout
CONV_TALL = (5, 128, 192, 64, 128)
CONV_NARROW = (2, 16, 48, 64, 48)


def sha(t):
    """sha256 of a device tensor's bytes, padding and border included"""
    return hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


@contextlib.contextmanager
def option(ltx, name, value):
    """one launcher switch moved for the block (None: left alone), then put back"""
    if value is None:
        yield
        return
    old = ltx.get_option(name)
    ltx.set_option(name, value)
    try:
        yield
    finally:
        ltx.set_option(name, old)


def _uniform(rng, shape, scale):
    return (rng.random(shape, dtype=np.float32) - 0.5) * scale


def _bf16(x, pad=0):
    """x [r][c] rounded to bf16 in the first c columns of a [r][c + pad] device tensor"""
    buf = torch.full((x.shape[0], x.shape[1] + pad), 3.0, dtype=torch.bfloat16, device="cuda")
    buf[:, :x.shape[1]] = torch.from_numpy(x).cuda().to(torch.bfloat16)
    return buf


def _f32(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()


def rowsplit_tile_cfg(ltx):
    """the tile choice of the row-split case: the split exists for the 192 x 256 kernel (75) only"""
    M, N, K = ROWSPLIT_SHAPE
    return ltx.gemm_dense_tile_cfg(M, N, K, flags=1, ncu=NCU)


def rowsplit_cases(ltx, ctx):
    M, N, K = ROWSPLIT_SHAPE
    rng = np.random.default_rng([SEED, M, N, K])
    A = _bf16(_uniform(rng, (M, K), 2.0), pad=8)
    B = _bf16(_uniform(rng, (N, K), 0.2))
    bias = _f32(_uniform(rng, (N,), 2.0))
    d = {}
    for name, value in (("rowsplit", None), ("rowsplit.gemm_rowsplit=0", 0)):
        out = torch.full((M + 2, N + 8), POISON, dtype=torch.float32, device="cuda")
        with option(ltx, "gemm_rowsplit", value):
            ctx._ck(ltx.lib.ltx_op_gemm_bf16(ctx._h, A.data_ptr(), A.stride(0), B.data_ptr(), B.stride(0), bias.data_ptr(), M, N, K, 0, -1,
                                             out.data_ptr(), out.stride(0), None, 0))
            torch.cuda.synchronize()
        d[f"{name}.{M}x{N}x{K}"] = sha(out)
    return d


def _grow_workspace(ctx):
    """The context's op workspace only grows, and a split count is shrunk to what fits it: a conv op brings it to the 64 MB it has wherever
    this runs behind other tests, so that the counts below do not depend on what ran before."""
    x = torch.zeros((1, 8, 8, 64), dtype=torch.bfloat16, device="cuda")
    w = torch.zeros((64, 27 * 64), dtype=torch.bfloat16, device="cuda")
    out = torch.empty((64, 64), dtype=torch.float32, device="cuda")
    ctx.op_conv3d(x, w, torch.zeros((64,), dtype=torch.float32, device="cuda"), out)
    torch.cuda.synchronize()


def _residual_norm(ltx, ctx, shape, fused, opt, value, name):
    M, N, K = shape
    rng = np.random.default_rng([SEED, M, N, K])
    A = _bf16(_uniform(rng, (M, K), 2.0), pad=8)
    B = _bf16(_uniform(rng, (N, K), 0.2))
    bias, gate = _f32(_uniform(rng, (N,), 2.0)), _f32(_uniform(rng, (N,), 2.0))
    scale, shift = _f32(_uniform(rng, (N,), 1.0)), _f32(_uniform(rng, (N,), 1.0))
    x0 = _f32(_uniform(rng, (M, N), 2.0))
    _grow_workspace(ctx)
    d = {}
    for key, v in ((name, None),) + (((f"{name}.{opt}={value}", value),) if opt else ()):
        x = torch.full((M + 2, N + 8), POISON, dtype=torch.float32, device="cuda")
        x[:M, :N] = x0
        xn = torch.full((M + 2, N + 8), POISON, dtype=torch.bfloat16, device="cuda")
        with option(ltx, opt, v):
            ctx._ck(ltx.lib.ltx_op_gemm_bf16_gated_residual_norm(ctx._h, A.data_ptr(), A.stride(0), B.data_ptr(), B.stride(0), bias.data_ptr(),
                                                                 gate.data_ptr(), 1.0, M, N, K, x.data_ptr(), x.stride(0), scale.data_ptr(),
                                                                 shift.data_ptr(), 1e-6, xn.data_ptr(), xn.stride(0), int(fused)))
            torch.cuda.synchronize()
        d[f"{key}.{M}x{N}x{K}.x"] = sha(x)
        d[f"{key}.{M}x{N}x{K}.xn"] = sha(xn)
    return d


def fewrow_cases(ltx, ctx):
    return _residual_norm(ltx, ctx, FEWROW_SHAPE, False, None, None, "fewrow")


def dtl_split_cases(ltx, ctx):
    return _residual_norm(ltx, ctx, DTL_SPLIT_SHAPE, True, "finish_norm", 0, "dtl_split")


def conv_cases(ltx, ctx, geom, name, options):
    """options: [(option name, value)], each recorded next to the default"""
    F, H, W, Cin, Cout = geom
    M = F * H * W
    rng = np.random.default_rng([SEED, F, H, W, Cin, Cout])
    x = _bf16(_uniform(rng, (M, Cin), 2.0)).view(F, H, W, Cin)
    w = _bf16(_uniform(rng, (Cout, 27 * Cin), 0.2))
    bias = _f32(_uniform(rng, (Cout,), 2.0))
    d = {}
    for opt, value in [(None, None)] + list(options):
        out = torch.full(((M + 2) * Cout,), POISON, dtype=torch.float32, device="cuda")  # the op's rows are Cout wide: two poisoned rows behind
        with option(ltx, opt, value):
            ctx.op_conv3d(x, w, bias, out)
            torch.cuda.synchronize()
        d[f"{name}{'' if opt is None else f'.{opt}={value}'}.{F}x{H}x{W}.{Cin}to{Cout}"] = sha(out)
    return d


CONV_CASES = [(CONV_TAIL, "conv_tail", [("conv_no_tail", 1)]), (CONV_TALL, "conv_tall", [("conv_tall", 0), ("conv_halo", 0)]),
              (CONV_NARROW, "conv_narrow", [])]


def all_cases(ltx, ctx):
    d = {}
    d.update(rowsplit_cases(ltx, ctx))
    d.update(fewrow_cases(ltx, ctx))
    d.update(dtl_split_cases(ltx, ctx))
    for geom, name, options in CONV_CASES:
        d.update(conv_cases(ltx, ctx, geom, name, options))
    return d


def expected_keys():
    keys = ["%s.%dx%dx%d" % (n, *ROWSPLIT_SHAPE) for n in ("rowsplit", "rowsplit.gemm_rowsplit=0")]
    keys += ["fewrow.%dx%dx%d.%s" % (*FEWROW_SHAPE, o) for o in ("x", "xn")]
    keys += ["%s.%dx%dx%d.%s" % (n, *DTL_SPLIT_SHAPE, o) for n in ("dtl_split", "dtl_split.finish_norm=0") for o in ("x", "xn")]
    for (F, H, W, Cin, Cout), name, options in CONV_CASES:
        keys += [f"{name}{s}.{F}x{H}x{W}.{Cin}to{Cout}" for s in [""] + [f".{o}={v}" for o, v in options]]
    return sorted(keys)
