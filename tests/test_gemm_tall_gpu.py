"""The 384 x 256 GEMM kernel (gemm_bf16_kernel_tall, tools/gen_gemm_asm_tall.py) through ltx_op_gemm_bf16(tile_cfg=76) and through the
launcher's default choice in a DiT forward (option "gemm_tall").

Op level, bit-exact: small-integer bf16 operands make every product and partial sum exact in f32, so the output must equal torch's f32
matmul + bias rounded to bf16; on random data tile_cfg 76 must equal tile_cfg 75 (the 192 x 256 kernel, which takes the same shapes)
bit for bit, with bias + GELU-tanh into a bf16 store and into an f32 store: one accumulator chain per output element, K ascending, and
the same epilogue arithmetic in both. M = 384 / 768 is one / two row tiles, N = 256 / 768 one / three column tiles (a grid that is no
multiple of 8), K = 64 .. 448 the prologue with fewer tiles than slots, every exit of the two-tile loop body and several wraps. The
activations and the output have padded leading dimensions, and the output a poisoned border.

Forward level: a 2-layer full-width DiT at 1536 tokens with the switch off and on gives bit-identical velocities and one denoise step
bit-identical latents."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

POISON = -777.0
KS = [64, 128, 192, 256, 320, 448]
MS = [384, 768]
NS = [256, 768]
GELU_TANH = 1


def _operands(rng, M, N, K, integer):
    if integer:
        X = rng.integers(-3, 4, (M, K)).astype(np.float32)
        W = rng.integers(-3, 4, (N, K)).astype(np.float32)
        b = rng.integers(-5, 6, (N,)).astype(np.float32)
    else:
        X = rng.standard_normal((M, K)).astype(np.float32)
        W = (rng.standard_normal((N, K)) * 0.05).astype(np.float32)
        b = rng.standard_normal((N,)).astype(np.float32)
    # activations with a padded leading dimension; the padding holds a value that would show in every result if it were read
    Xd = torch.full((M, K + 8), 3.0, dtype=torch.bfloat16, device="cuda")
    Xd[:, :K] = torch.from_numpy(X).to(torch.bfloat16).cuda()
    return Xd[:, :K], torch.from_numpy(W).to(torch.bfloat16).cuda(), torch.from_numpy(b).cuda()


def _launch(ltx, ctx, X, W, b, act, cfg, out):
    """ltx_op_gemm_bf16 on views with padded leading dimensions (Context.op_gemm takes contiguous tensors only)"""
    M, K = X.shape
    f32 = out.dtype == torch.float32
    ctx._ck(ltx.lib.ltx_op_gemm_bf16(ctx._h, X.data_ptr(), X.stride(0), W.data_ptr(), W.stride(0), b.data_ptr(), M, W.shape[0], K, act, cfg,
                                     out.data_ptr() if f32 else None, out.stride(0) if f32 else 0, None if f32 else out.data_ptr(),
                                     0 if f32 else out.stride(0)))


def _run(ltx, ctx, X, W, b, act, cfg, dtype):
    """out [M + 2][N + 8], poisoned: the launch may write [:M, :N]"""
    M, N = X.shape[0], W.shape[0]
    buf = torch.full((M + 2, N + 8), POISON, dtype=dtype, device="cuda")
    _launch(ltx, ctx, X, W, b, act, cfg, buf[:M, :N])
    torch.cuda.synchronize()
    return buf


def _border_untouched(buf, M, N):
    return bool((buf[M:] == POISON).all() and (buf[:, N:] == POISON).all())


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("M", MS)
def test_tall_is_exact_on_integer_data(ltx, gpu_ctx, M, N, K):
    X, W, b = _operands(np.random.default_rng(M * 7 + N * 3 + K), M, N, K, integer=True)
    buf = _run(ltx, gpu_ctx, X, W, b, 0, 76, torch.bfloat16)
    ref = (X.float() @ W.float().T + b).to(torch.bfloat16)
    assert torch.equal(buf[:M, :N], ref), f"{(buf[:M, :N].float() - ref.float()).abs().max().item()}"
    assert _border_untouched(buf, M, N)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("M", MS)
def test_tall_equals_the_192x256_kernel_on_random_data(ltx, gpu_ctx, M, N, K, dtype):
    X, W, b = _operands(np.random.default_rng(M + N * 5 + K * 11), M, N, K, integer=False)
    got = _run(ltx, gpu_ctx, X, W, b, GELU_TANH, 76, dtype)
    ref = _run(ltx, gpu_ctx, X, W, b, GELU_TANH, 75, dtype)
    bits = torch.int16 if dtype == torch.bfloat16 else torch.int32
    assert torch.equal(got.view(bits), ref.view(bits)), f"{(got[:M, :N].float() - ref[:M, :N].float()).abs().max().item()}"
    assert _border_untouched(got, M, N) and _border_untouched(ref, M, N)
    lin = X.float() @ W.float().T + b                                  # not a bound on the kernel: the data is not degenerate
    assert float(lin.abs().mean()) > 0.1 and bool(torch.isfinite(got[:M, :N].float()).all())
    assert float((got[:M, :N].float() - torch.nn.functional.gelu(lin, approximate="tanh")).abs().max()) < 0.1


def test_refused_shape_raises_before_anything_is_launched(ltx, gpu_ctx):
    M, N, K = 200, 256, 128
    X, W, b = _operands(np.random.default_rng(5), M, N, K, integer=True)
    buf = torch.full((M + 2, N + 8), POISON, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(ltx.LTXError, match="384x256 kernel"):
        _launch(ltx, gpu_ctx, X, W, b, 0, 76, buf[:M, :N])
    torch.cuda.synchronize()
    assert bool((buf == POISON).all())


@pytest.fixture(scope="module")
def two_layer(ltx):
    ctx = ltx.Context(0)
    cfg = ltx.default_transformer_config(num_layers=2, num_attention_heads=32, cross_attention_dim=32 * 128, caption_channels=256)
    ctx.dit_init_synthetic(cfg, seed=7)
    yield ctx
    ctx.close()


def test_forward_and_denoise_step_are_bit_identical_with_the_switch(ltx, two_layer):
    ctx, (F, H, W) = two_layer, (4, 16, 24)
    T, S = F * H * W, 64
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    if 256 % ncu == 0:   # the FFN-up projection of this forward (GELU, bf16 store) is whole rounds of 384 x 256 tiles: the graph takes the kernel
        assert ltx.gemm_dense_tile_cfg(T, 16384, 4096, act=GELU_TANH, flags=2, ncu=ncu) == 76
    lat = torch.empty((1, T, 128), dtype=torch.bfloat16, device="cuda")
    ctx.op_fill_normal_bf16(lat, seed=3)
    cx = torch.empty((1, S, 256), dtype=torch.bfloat16, device="cuda")
    ctx.op_fill_normal_bf16(cx, seed=4)
    ts = torch.full((1,), 0.7, dtype=torch.float32, device="cuda")
    vel, stepped = {}, {}
    sig = np.array([1.0, 0.8], np.float32)
    noise = torch.randn((1, 128, F, H, W), generator=torch.Generator().manual_seed(1)).cuda()
    for on in (0, 1):
        with ctx.options(gemm_tall=on):
            vel[on] = torch.empty((1, T, 128), dtype=torch.float32, device="cuda")
            ctx.dit_forward_dev(lat, cx, ts, None, F, H, W, vel[on], ctx_version=5)
            torch.cuda.synchronize()
            stepped[on] = noise.clone()
            ctx.denoise_dev(stepped[on], sig, cx, None, F, H, W, ctx_version=5)
            torch.cuda.synchronize()
    assert bool(torch.isfinite(vel[1]).all()) and float(vel[1].abs().mean()) > 0
    assert torch.equal(vel[0].view(torch.int32), vel[1].view(torch.int32))
    assert torch.equal(stepped[0].view(torch.int32), stepped[1].view(torch.int32)) and not torch.equal(stepped[1], noise)
