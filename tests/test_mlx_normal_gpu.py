"""The grouped MLX-normal kernel (csrc/noise.hip) through ltx_op_mlx_normal_group and ltx_mlx_random_normal_dev. The integer half - the
threefry2x32-20 counters and the layout of mlx_random_bits for even and odd counts - is exact against the oracle; the float half is
compared with the host generator ltx_mlx_random_normal, whose arithmetic the kernel restates operation by operation, so that a value can
differ only where the two logf differ in their last place: the tolerance is the project's own for this pipeline (tests/test_host_logic.py,
"libm logf vs numpy log: <= 1 ulp apart"). Sizes: below, at and above one wave (63, 64, 65), one workgroup of 256 counters = 512 values
(511, 513), several workgroups (16128 = the audio draw 8 x 126 x 16, 49153), odd sizes with their middle element."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
SIZES = [1, 2, 3, 63, 64, 65, 255, 256, 257, 511, 513, 16128, 49153]
RTOL, ATOL = 2e-6, 1e-7
GUARD = 0x5A5A5A5A


def key_of(ltx, seed, draw):
    return [int(v) for v in ltx.mlx_draw_key(seed, draw)]


def guarded(n, pad=8):
    """n int32 words and `pad` guard words after them."""
    return torch.full((n + pad,), GUARD, dtype=torch.int32, device="cuda")


def bits(t, n):
    return t[:n].cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("n", SIZES)
def test_raw_bits_equal_the_oracle(ltx, oracle, gpu_ctx, n):
    key = key_of(ltx, 42, 1)
    buf = guarded(n)
    gpu_ctx.op_mlx_normal_group([dict(key=key, dst=buf, n=n, raw_bits=True)])
    torch.cuda.synchronize()
    want = oracle.mlx_random_bits((np.uint32(key[0]), np.uint32(key[1])), n)
    got = bits(buf, n)
    assert np.array_equal(got, want)
    if n % 2:  # the middle element: counter (half, 0), word 0 alone
        a, _ = oracle.threefry2x32(key, np.array([n // 2], np.uint32), np.array([0], np.uint32))
        assert got[n // 2] == a[0]
    assert (buf[n:] == GUARD).all()


def test_a_group_equals_single_launches_and_stays_inside_its_buffers(ltx, gpu_ctx):
    sizes = [513, 64, 0, 16128, 257]  # odd and even, an empty job in the middle, more than one workgroup
    keys = [key_of(ltx, 7, d) for d in range(5)]
    for raw in (True, False):
        grouped = [guarded(n) for n in sizes]
        single = [guarded(n) for n in sizes]
        jobs = lambda bufs: [dict(key=k, dst=b, n=n, raw_bits=raw, scale=0.75) for k, b, n in zip(keys, bufs, sizes)]  # noqa: E731
        gpu_ctx.op_mlx_normal_group(jobs(grouped))
        for j in jobs(single):
            gpu_ctx.op_mlx_normal_group([j])
        torch.cuda.synchronize()
        for g, s, n in zip(grouped, single, sizes):
            assert torch.equal(g, s)
            assert (g[n:] == GUARD).all()
            assert n == 0 or not (g[:n] == GUARD).all()
    # a NULL destination is fine for an empty job, and no job at all is valid
    gpu_ctx.op_mlx_normal_group([dict(key=keys[0], dst=None, n=0)])
    gpu_ctx.op_mlx_normal_group([])


def test_more_jobs_than_one_launch_holds(ltx, gpu_ctx):
    """70 jobs: the 64 of one launch and a second launch for the rest."""
    n = 33
    bufs = [guarded(n) for _ in range(70)]
    gpu_ctx.op_mlx_normal_group([dict(key=key_of(ltx, 3, d), dst=b, n=n) for d, b in enumerate(bufs)])
    torch.cuda.synchronize()
    for d in (0, 63, 64, 69):
        want = ltx.mlx_random_normal(3, (n,), d)
        np.testing.assert_allclose(bufs[d][:n].cpu().numpy().view(np.float32), want, rtol=RTOL, atol=ATOL)
        assert (bufs[d][n:] == GUARD).all()


def test_normals_against_the_host_generator(ltx, gpu_ctx):
    equal = total = 0
    for seed, draw, n in [(42, 0, 49153), (42, 1, 16128), (2**40 + 5, 7, 513), (0, 0, 3), (9, 2, 1)]:
        out = torch.zeros(n, device="cuda")
        gpu_ctx.mlx_random_normal_dev(seed, out, draw)
        torch.cuda.synchronize()
        got, want = out.cpu().numpy(), ltx.mlx_random_normal(seed, (n,), draw)
        assert np.isfinite(got).all()
        np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL)
        equal += int((got.view(np.uint32) == want.view(np.uint32)).sum())
        total += n
    share = equal / total
    print(f"device normals bit-equal to the host generator: {equal} of {total} ({100 * share:.4f} %)")
    record = os.environ.get("LTX_NOISE_SHARE_FILE")  # measured, not asserted: profiles/noise_bench.txt records it
    if record:
        with open(record, "w") as f:
            f.write(f"{equal} {total} {share:.6f}\n")


def test_scale_is_one_more_f32_multiply(ltx, gpu_ctx):
    n = 4099
    plain, one, scaled = (torch.zeros(n, device="cuda") for _ in range(3))
    key = key_of(ltx, 11, 0)
    s = 0.909375
    gpu_ctx.op_mlx_normal_group([dict(key=key, dst=plain), dict(key=key, dst=one, scale=1.0), dict(key=key, dst=scaled, scale=s)])
    torch.cuda.synchronize()
    p = plain.cpu().numpy()
    assert np.array_equal(one.cpu().numpy().view(np.uint32), p.view(np.uint32))
    assert np.array_equal(scaled.cpu().numpy().view(np.uint32), (np.float32(s) * p).astype(np.float32).view(np.uint32))


def test_refusals_write_nothing(ltx, gpu_ctx):
    buf = guarded(64)
    ok = dict(key=[1, 2], dst=buf, n=64)
    for bad in (dict(key=[1, 2], dst=buf, n=-1), dict(key=[1, 2], dst=buf, n=2**31), dict(key=[1, 2], dst=None, n=5)):
        with pytest.raises(ltx.LTXError) as e:
            gpu_ctx.op_mlx_normal_group([ok, bad])  # the good job first: nothing of the call may run
        assert e.value.case == "invalidConfiguration"
    with pytest.raises(ltx.LTXError) as e:
        gpu_ctx.op_mlx_normal_group([ok], n_jobs=-1)
    assert e.value.case == "invalidConfiguration"
    with pytest.raises(ltx.LTXError):
        gpu_ctx.mlx_random_normal_dev(1, buf.view(torch.float32), draw_index=-1)
    torch.cuda.synchronize()
    assert (buf == GUARD).all()
