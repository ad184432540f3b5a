"""The fused q|k + V projection (gemm_bf16_kernel_qkv, 192 x 384 tiles, tools/gen_gemm_asm_qkv.py) through ltx_op_qkv_projection and
through the DiT graph's switch "qkv_fused".

Op level, bit-exact: small-integer bf16 operands make every product and partial sum exact in f32, so qk_out must equal torch's f32
matmul rounded to bf16 and vt_out the same reference transposed; on random data the fused launch must equal the two-launch path bit
for bit (one accumulator chain per output element, K ascending, in both). K = 64 .. 448 is every exit of the two-tile loop body, the
prologue with fewer tiles than slots and several wraps; D = 128 / 384 is one / three column tiles (a grid that is no multiple of 8);
576 rows is three row tiles; the activations and both outputs have padded leading dimensions, and both outputs a poisoned border.

Forward level: a 2-layer DiT with the switch off and on gives bit-identical velocities and one denoise step bit-identical latents."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

POISON = -777.0
KS = [64, 128, 192, 256, 320, 448]
SHAPES = [(192, 192, 128), (192, 192, 384), (576, 576, 128), (576, 576, 384), (384, 192, 128), (384, 192, 384)]   # rows, rows per batch, D


def _padded(x, pad, dtype):
    """x [r][c] in the first c columns of a [r][c + pad] device tensor (leading dimension c + pad); the padding holds a value that
    would show in every result if it were read."""
    buf = torch.full((x.shape[0], x.shape[1] + pad), 3.0, dtype=dtype, device="cuda")
    buf[:, :x.shape[1]] = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dtype).cuda()
    return buf


def _operands(rng, rows, D, K, integer):
    if integer:
        X = rng.integers(-3, 4, (rows, K)).astype(np.float32)
        Wqk = rng.integers(-3, 4, (2 * D, K)).astype(np.float32)
        Wv = rng.integers(-3, 4, (D, K)).astype(np.float32)
        bqk = rng.integers(-5, 6, (2 * D,)).astype(np.float32)
        bv = rng.integers(-5, 6, (D,)).astype(np.float32)
    else:
        X = rng.standard_normal((rows, K)).astype(np.float32)
        Wqk = (rng.standard_normal((2 * D, K)) * 0.05).astype(np.float32)
        Wv = (rng.standard_normal((D, K)) * 0.05).astype(np.float32)
        bqk = rng.standard_normal((2 * D,)).astype(np.float32)
        bv = rng.standard_normal((D,)).astype(np.float32)
    # (the weights are dense [out][K], as a Linear holds them: the entry point takes no leading dimension for them)
    return dict(X=_padded(X, 8, torch.bfloat16), Wqk=_padded(Wqk, 0, torch.bfloat16), Wv=_padded(Wv, 0, torch.bfloat16),
                bqk=torch.from_numpy(bqk).cuda(), bv=torch.from_numpy(bv).cuda())


def _outputs(rows, rpb, D):
    """qk_out [rows + 2][2 D + 8] and vt_out [rows / rpb][D + 1][rpb + 4], poisoned: the launch may write [:rows, :2 D] and [:, :D, :rpb]."""
    qk = torch.full((rows + 2, 2 * D + 8), POISON, dtype=torch.bfloat16, device="cuda")
    vt = torch.full(((rows // rpb) * D + 1, rpb + 4), POISON, dtype=torch.bfloat16, device="cuda")
    return qk, vt


def _run(ctx, dev, rows, rpb, D, fused):
    qk, vt = _outputs(rows, rpb, D)
    ctx.op_qkv_projection(dev["X"], dev["Wqk"], dev["bqk"], dev["Wv"], dev["bv"], qk, vt, rows=rows, rows_per_batch=rpb, fused=fused)
    torch.cuda.synchronize()
    return qk, vt


def _border_untouched(qk, vt, rows, rpb, D):
    return bool((qk[rows:] == POISON).all() and (qk[:, 2 * D:] == POISON).all() and (vt[(rows // rpb) * D:] == POISON).all() and
                (vt[:, rpb:] == POISON).all())


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("rows,rpb,D", SHAPES)
def test_fused_is_exact_on_integer_data(gpu_ctx, rows, rpb, D, K):
    dev = _operands(np.random.default_rng(rows * 7 + D * 3 + K + rpb), rows, D, K, integer=True)
    qk, vt = _run(gpu_ctx, dev, rows, rpb, D, fused=True)
    X = dev["X"][:, :K].float()
    ref_qk = (X @ dev["Wqk"].float().T + dev["bqk"]).to(torch.bfloat16)
    ref_v = (X @ dev["Wv"].float().T + dev["bv"]).to(torch.bfloat16)              # [rows][D]
    ref_vt = ref_v.view(rows // rpb, rpb, D).transpose(1, 2)                      # [batch][D][rpb]
    assert torch.equal(qk[:rows, :2 * D], ref_qk), f"q|k: {(qk[:rows, :2 * D].float() - ref_qk.float()).abs().max().item()}"
    got_vt = vt[:(rows // rpb) * D].view(rows // rpb, D, rpb + 4)[:, :, :rpb]
    assert torch.equal(got_vt, ref_vt), f"V^T: {(got_vt.float() - ref_vt.float()).abs().max().item()}"
    assert _border_untouched(qk, vt, rows, rpb, D)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("rows,rpb,D", SHAPES)
def test_fused_equals_two_launches_on_random_data(gpu_ctx, rows, rpb, D, K):
    dev = _operands(np.random.default_rng(rows + D * 5 + K * 11 + rpb), rows, D, K, integer=False)
    qk1, vt1 = _run(gpu_ctx, dev, rows, rpb, D, fused=True)
    qk0, vt0 = _run(gpu_ctx, dev, rows, rpb, D, fused=False)
    assert torch.equal(qk1.view(torch.int16), qk0.view(torch.int16)) and torch.equal(vt1.view(torch.int16), vt0.view(torch.int16))
    assert _border_untouched(qk1, vt1, rows, rpb, D) and _border_untouched(qk0, vt0, rows, rpb, D)
    ref = dev["X"][:, :K].float() @ dev["Wqk"].float().T + dev["bqk"]                    # not a bound on the kernel: the data is not degenerate
    assert float(ref.abs().mean()) > 0.1 and bool(torch.isfinite(qk1[:rows, :2 * D].float()).all())


def test_fallback_shape_runs_unfused_and_is_refused_fused(ltx, gpu_ctx):
    rows, D, K = 200, 128, 128
    dev = _operands(np.random.default_rng(5), rows, D, K, integer=True)
    qk, vt = _run(gpu_ctx, dev, rows, rows, D, fused=False)
    X = dev["X"][:, :K].float()
    assert torch.equal(qk[:rows, :2 * D], (X @ dev["Wqk"].float().T + dev["bqk"]).to(torch.bfloat16))
    assert torch.equal(vt[:D, :rows], (X @ dev["Wv"].float().T + dev["bv"]).to(torch.bfloat16).T)
    assert _border_untouched(qk, vt, rows, rows, D)
    qk, vt = _outputs(rows, rows, D)
    with pytest.raises(ltx.LTXError, match="fused q\\|k \\+ V kernel"):
        gpu_ctx.op_qkv_projection(dev["X"], dev["Wqk"], dev["bqk"], dev["Wv"], dev["bv"], qk, vt, rows=rows, rows_per_batch=rows, fused=True)
    torch.cuda.synchronize()
    assert bool((qk == POISON).all() and (vt == POISON).all())   # refused before anything was launched


# heads = 8 (D = 1024): at 384 tokens neither of the two launches splits its K = 1024 reduction, so the graph does take the fused launch
# (the full-width model at 384 tokens keeps its two launches: they split K). heads = 32 at 1536 tokens is the benchmark's shape.
@pytest.fixture(scope="module", params=[(8, 6, 8, 8), (32, 4, 16, 24)], ids=["D1024-384tok", "D4096-1536tok"])
def two_layer(request, ltx):
    heads, F, H, W = request.param
    ctx = ltx.Context(0)
    cfg = ltx.default_transformer_config(num_layers=2, num_attention_heads=heads, cross_attention_dim=heads * 128, caption_channels=256)
    ctx.dit_init_synthetic(cfg, seed=7)
    yield ctx, F, H, W
    ctx.close()


def _gemm_launches(ctx):
    return ctx.prof_collect(0, reset=True)["launches"]


def test_forward_and_denoise_step_are_bit_identical_with_the_switch(ltx, two_layer):
    ctx, F, H, W = two_layer
    T, S = F * H * W, 64
    lat = torch.empty((1, T, 128), dtype=torch.bfloat16, device="cuda")
    ctx.op_fill_normal_bf16(lat, seed=3)
    cx = torch.empty((1, S, 256), dtype=torch.bfloat16, device="cuda")
    ctx.op_fill_normal_bf16(cx, seed=4)
    ts = torch.full((1,), 0.7, dtype=torch.float32, device="cuda")
    vel, launches, stepped = {}, {}, {}
    sig = np.array([1.0, 0.8], np.float32)
    noise = torch.randn((1, 128, F, H, W), generator=torch.Generator().manual_seed(1)).cuda()
    warm = torch.empty((1, T, 128), dtype=torch.float32, device="cuda")
    ctx.dit_forward_dev(lat, cx, ts, None, F, H, W, warm, ctx_version=5)   # the text K/V of this context version are cached from here on
    ctx.prof_enable(True)
    try:
        for on in (0, 1):
            with ctx.options(qkv_fused=on):
                vel[on] = torch.empty((1, T, 128), dtype=torch.float32, device="cuda")
                _gemm_launches(ctx)
                ctx.dit_forward_dev(lat, cx, ts, None, F, H, W, vel[on], ctx_version=5)
                torch.cuda.synchronize()
                launches[on] = _gemm_launches(ctx)
                stepped[on] = noise.clone()
                ctx.denoise_dev(stepped[on], sig, cx, None, F, H, W, ctx_version=5)
                torch.cuda.synchronize()
    finally:
        ctx.prof_enable(False)
    assert launches[0] - launches[1] == 2, launches   # one GEMM launch fewer per block: the graph did take the fused kernel
    assert bool(torch.isfinite(vel[1]).all()) and float(vel[1].abs().mean()) > 0
    assert torch.equal(vel[0].view(torch.int32), vel[1].view(torch.int32))
    assert torch.equal(stepped[0].view(torch.int32), stepped[1].view(torch.int32)) and not torch.equal(stepped[1], noise)
