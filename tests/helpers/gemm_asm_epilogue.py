"""Every epilogue form of the three GEMM kernels with a generated main loop (csrc/gemm_asm_tiles.inc) as one sha256 per output buffer,
through ltx_op_gemm_tile (192 x 256: tile_cfg 75, 384 x 256: 76) and ltx_op_qkv_projection. tests/test_gemm_asm_epilogue_gpu.py
compares them with tests/golden/gemm_asm_epilogue_digests.json, which

    LTX_LIB=<libltxhip.so with the kernels of the commit to pin> python tests/helpers/gemm_asm_epilogue.py --record [FILE]

writes: the golden file is recorded from a library built BEFORE a change to the epilogues, never from the code under test. The plain
stores are picked once per launch from a list of instantiated variants and go through per-lane row pointers; what can go wrong there is
a wrong variant for a combination of outputs, a wrong row / column base or stride, and another order of floating-point operations:

  shapes    one tile and 2 x 2 tiles per kernel (192 / 384 rows for 75 and q|k|v, 384 / 768 for 76; 256 / 512 columns; q|k|v with
            D = 128 / 256, i.e. 256 / 512 q|k columns and half as many of V), K = 64, 128, 192 (one, two, three K-tiles), every output
            with a leading dimension of N + 8 and a poisoned border that the digest covers
  variants  bf16; GELU-tanh -> bf16; f32; f32 + bf16 (the instantiated ones) and SiLU -> bf16, GELU-tanh -> f32 rounded through bf16
            (the generic body), each with and without a column bias; a per-row bias on 75
  residual  75: gate vector of one batch element, of two batch elements of 192 rows, through a row map, scalar gate; in place and
            from another buffer, with and without the bf16 copy
  split-K   75: two K ranges with f32 and with bf16 partial tiles
  overflow  weights scaled so that the pre-activation values pass +-40: the exponent of GELU-tanh overflows and the result must be
            -0 or x"""
import ctypes
import hashlib
import json
import os
import sys

import numpy as np
import torch

SEED = 31
POISON = -777.0
NONE, GELU_TANH, SILU = 0, 1, 2
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "golden", "gemm_asm_epilogue_digests.json")
SIZES = {75: {"1x1": (192, 256), "2x2": (384, 512)}, 76: {"1x1": (384, 256), "2x2": (768, 512)}}
KS = (64, 128, 192)
# name: (activation, round_bf16, f32 output, bf16 output)
VARIANTS = {"bf16": (NONE, 0, False, True), "gelu_bf16": (GELU_TANH, 0, False, True), "f32": (NONE, 0, True, False),
            "f32_bf16": (NONE, 0, True, True), "silu_bf16": (SILU, 0, False, True), "gelu_round_f32": (GELU_TANH, 1, True, False)}
QKV_SIZES = {"1x1": (192, 192, 128), "2x2": (384, 192, 256)}   # rows, rows per batch, D
RESID_FORMS = ("gate_one_batch", "gate_two_batches", "gate_rowmap", "gate_scalar_src_mirror")


def sha(t):
    return hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def _bf16(x, pad=8):
    buf = torch.full((x.shape[0], x.shape[1] + pad), 3.0, dtype=torch.bfloat16, device="cuda")
    buf[:, :x.shape[1]] = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16).cuda()
    return buf


def _f32(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()


def _out(M, N, dtype):
    return torch.full((M + 2, N + 8), POISON, dtype=dtype, device="cuda")


def launch(ltx, ctx, cfg, A, B, M, N, K, **kw):
    """one ltx_op_gemm_tile launch; kw: the fields of ltx_gemm_tile_launch, tensors for the pointers"""
    l = ltx.GemmTileLaunch()
    l.struct_size = ctypes.sizeof(ltx.GemmTileLaunch)
    l.tile_cfg, l.A, l.lda, l.B, l.ldb, l.M, l.N, l.K = cfg, A.data_ptr(), A.stride(0), B.data_ptr(), B.stride(0), M, N, K
    l.split_k, l.gate_scalar = 1, 1.0
    for k, v in kw.items():
        if isinstance(v, torch.Tensor):
            setattr(l, k, v.data_ptr())
            if k in ("out_f32", "out_bf16", "resid_src"):
                setattr(l, {"out_f32": "ld_f32", "out_bf16": "ld_bf16", "resid_src": "ld_resid"}[k], v.stride(0))
        elif v is not None:
            setattr(l, k, v)
    ctx._ck(ltx.lib.ltx_op_gemm_tile(ctx._h, ctypes.byref(l)))
    torch.cuda.synchronize()


def _operands(tag, M, N, K, wscale=0.05):
    rng = np.random.default_rng([SEED, *tag, M, N, K])
    return rng, _bf16(rng.standard_normal((M, K))), _bf16(rng.standard_normal((N, K)) * wscale, pad=0), _f32(rng.standard_normal((N,)))


def plain_cases(ltx, ctx, cfg, size):
    """every variant x K x (column bias, none) on one shape of one kernel"""
    M, N = SIZES[cfg][size]
    d = {}
    for K in KS:
        _, A, B, bias = _operands((cfg, 0), M, N, K)
        for name, (act, rnd, f32, bf16) in VARIANTS.items():
            for bname, b in (("bias", bias), ("nobias", None)):
                of, ob = (_out(M, N, torch.float32) if f32 else None), (_out(M, N, torch.bfloat16) if bf16 else None)
                launch(ltx, ctx, cfg, A, B, M, N, K, act=act, round_bf16=rnd, bias_n=b, out_f32=of, out_bf16=ob)
                for oname, o in (("f32", of), ("bf16", ob)):
                    if o is not None:
                        d[f"cfg{cfg}.{size}.K{K}.{name}.{bname}.out_{oname}"] = sha(o)
    return d


def row_bias_cases(ltx, ctx):
    d = {}
    for size, (M, N) in SIZES[75].items():
        rng, A, B, bias = _operands((75, 1), M, N, 128)
        bm = _f32(rng.standard_normal((M,)))
        for name in ("bf16", "f32_bf16"):
            act, rnd, f32, bf16 = VARIANTS[name]
            of, ob = (_out(M, N, torch.float32) if f32 else None), _out(M, N, torch.bfloat16)
            launch(ltx, ctx, 75, A, B, M, N, 128, act=act, bias_n=bias, bias_m=bm, out_f32=of, out_bf16=ob)
            d[f"cfg75.{size}.rowbias.{name}.out_bf16"] = sha(ob)
            if of is not None:
                d[f"cfg75.{size}.rowbias.{name}.out_f32"] = sha(of)
    return d


def resid_cases(ltx, ctx, form):
    """the residual + gate epilogue of the 192 x 256 kernel on 2 x 2 tiles"""
    M, N = SIZES[75]["2x2"]
    d = {}
    for K in (64, 192):
        rng, A, B, bias = _operands((75, 2, RESID_FORMS.index(form)), M, N, K)
        x = _out(M, N, torch.float32)
        x[:M, :N] = _f32(rng.standard_normal((M, N), dtype=np.float32))
        kw = dict(resid=1, bias_n=bias, out_f32=x)
        mirror = None
        if form == "gate_one_batch":
            kw.update(gate=_f32(rng.standard_normal((N,))), rows_per_batch=M)
        elif form == "gate_two_batches":
            mirror = _out(M, N, torch.bfloat16)
            kw.update(gate=_f32(rng.standard_normal((2, N + 16))), gate_bstride=N + 16, rows_per_batch=192, out_bf16=mirror)
        elif form == "gate_rowmap":
            rowmap = torch.from_numpy(rng.integers(0, 3, size=(M,)).astype(np.int32)).cuda()
            kw.update(gate=_f32(rng.standard_normal((3, N))), gate_bstride=N, gate_rowmap=rowmap, rows_per_batch=M)
        else:
            mirror = _out(M, N, torch.bfloat16)
            src = _f32(rng.standard_normal((M, N + 16), dtype=np.float32))
            kw.update(gate_scalar=0.75, resid_src=src, out_bf16=mirror, bias_n=None)
        launch(ltx, ctx, 75, A, B, M, N, K, **kw)
        d[f"cfg75.resid.{form}.K{K}.x"] = sha(x)
        if mirror is not None:
            d[f"cfg75.resid.{form}.K{K}.mirror"] = sha(mirror)
    return d


def splitk_cases(ltx, ctx, partial):
    """two K ranges of the 192 x 256 kernel; partial: "f32" / "bf16" tiles across the workspace"""
    d = {}
    for size, (M, N) in SIZES[75].items():
        for K in (128, 192):
            _, A, B, bias = _operands((75, 3), M, N, K)
            of, ob = _out(M, N, torch.float32), _out(M, N, torch.bfloat16)
            launch(ltx, ctx, 75, A, B, M, N, K, split_k=2, split_bf16=int(partial == "bf16"), bias_n=bias, out_f32=of, out_bf16=ob)
            d[f"cfg75.{size}.K{K}.split2_{partial}.out_f32"] = sha(of)
            d[f"cfg75.{size}.K{K}.split2_{partial}.out_bf16"] = sha(ob)
    return d


def overflow_cases(ltx, ctx, cfg):
    """GELU-tanh -> bf16 on pre-activation values beyond +-40; also returns (largest stored value, number of stored -0)"""
    M, N = SIZES[cfg]["1x1"]
    _, A, B, bias = _operands((cfg, 4), M, N, 64, wscale=1.5)   # pre-activation std = 1.5 * sqrt(64) = 12 over 10^5 elements
    ob = _out(M, N, torch.bfloat16)
    launch(ltx, ctx, cfg, A, B, M, N, 64, act=GELU_TANH, bias_n=bias, out_bf16=ob)
    inner = ob[:M, :N]
    neg_zero = int((inner.view(torch.int16) == -32768).sum())
    return {f"cfg{cfg}.overflow.gelu_bf16": sha(ob)}, float(inner.float().max()), neg_zero


def qkv_cases(ctx, size):
    rows, rpb, D = QKV_SIZES[size]
    d = {}
    for K in KS:
        rng = np.random.default_rng([SEED, 5, rows, D, K])
        X, Wqk, Wv = _bf16(rng.standard_normal((rows, K))), _bf16(rng.standard_normal((2 * D, K)) * 0.05, pad=0), _bf16(rng.standard_normal((D, K)) * 0.05, pad=0)
        bqk, bv = _f32(rng.standard_normal((2 * D,))), _f32(rng.standard_normal((D,)))
        for bname, (b1, b2) in (("bias", (bqk, bv)), ("nobias", (None, None))):
            qk = _out(rows, 2 * D, torch.bfloat16)
            vt = torch.full(((rows // rpb) * D + 1, rpb + 4), POISON, dtype=torch.bfloat16, device="cuda")
            ctx.op_qkv_projection(X, Wqk, b1, Wv, b2, qk, vt, rows=rows, rows_per_batch=rpb, fused=True)
            torch.cuda.synchronize()
            d[f"qkv.{size}.K{K}.{bname}.qk_out"] = sha(qk)
            d[f"qkv.{size}.K{K}.{bname}.vt_out"] = sha(vt)
    return d


def all_cases(ltx, ctx):
    d = {}
    for cfg in SIZES:
        for size in SIZES[cfg]:
            d.update(plain_cases(ltx, ctx, cfg, size))
        d.update(overflow_cases(ltx, ctx, cfg)[0])
    d.update(row_bias_cases(ltx, ctx))
    for form in RESID_FORMS:
        d.update(resid_cases(ltx, ctx, form))
    for partial in ("f32", "bf16"):
        d.update(splitk_cases(ltx, ctx, partial))
    for size in QKV_SIZES:
        d.update(qkv_cases(ctx, size))
    return d


if __name__ == "__main__":
    assert sys.argv[1:2] == ["--record"] and len(sys.argv) <= 3, __doc__
    target = sys.argv[2] if len(sys.argv) == 3 else GOLDEN
    import importlib
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
    ltx = importlib.import_module("ltx-video-swift-mlx_amd")
    ctx = ltx.Context(0)
    digests = all_cases(ltx, ctx)
    ctx.close()
    with open(target, "w") as f:
        json.dump({"seed": SEED, "digests": dict(sorted(digests.items()))}, f, indent=0)
        f.write("\n")
    print(f"{len(digests)} digests from {ltx._lib.SO_PATH} -> {os.path.normpath(target)}")
