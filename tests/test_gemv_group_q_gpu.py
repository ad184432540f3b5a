"""The grouped small-M gemv on affine-quantised weights (gemv_group_q_kernel, csrc/gemm.hip) through ltx_op_gemv_group_q: every job is
BIT-EQUAL to ltx_op_gemv_f32 on W = bf16(q * scale + bias), the matrix the library's de-quantiser writes (numpy builds it here: q <= 255
times a bf16 scale is exact in f32, so the one rounding of the sum and the one to bf16 are the same in numpy and on the device).
MLX affine layout, group 64 along K; 8 bits one code per byte, 4 bits two per byte with the even element in the low nibble.

Shapes: K = 64 (eight lanes work), 256, 320 (a ragged only trip), 576 (one whole trip and a ragged one), 2048, 4096 and 4096 + 192 (every
chunk size and a ragged trip behind the largest); N = 1, 3, 4, 130, 1024 (tails inside a workgroup and at job boundaries); M = 1, 2, 3, 8
(both MMAX instances); 1, 6 and 8 jobs; an N = 0 job; outputs inside a wider NaN-filled row; both activations; both ways the scale /
bias pair reaches its eight lanes (option "gemvq_sb")."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
SILU = 2
# (N, K, activation, bias, integer-valued activations)
SIX = ((1, 64, 0, True, True), (130, 256, SILU, True, False), (3, 320, 0, False, False), (1024, 576, SILU, True, False), (4, 2048, 0, True, True),
       (130, 4096 + 192, SILU, False, False))
EIGHT = SIX + ((3, 4096, 0, True, False), (0, 128, SILU, False, False))


def dequant(oracle, q, scales, biases):
    """bf16(q * scale + bias) per 64-wide group along K, in numpy."""
    N, K = q.shape
    return oracle.bf16_round(q.reshape(N, K // 64, 64).astype(np.float32) * scales[:, :, None] + biases[:, :, None]).reshape(N, K)


def pack(q, bits):
    if bits == 8:
        return q.astype(np.uint8)
    return (q[:, 0::2] | (q[:, 1::2] << 4)).astype(np.uint8)  # the even element in the low nibble


def to_bf16(ltx, a):
    return torch.from_numpy(ltx.f32_to_bf16_bits(np.ascontiguousarray(a, dtype=np.float32)).astype(np.int16)).cuda().view(torch.bfloat16)


def make_job(ltx, oracle, rng, bits, M, N, K, in_act, bias, integer, pad=3, q=None, scales=None, biases=None):
    """Random codes, bf16 scales / biases and activations; `out` is a view into the middle of a wider NaN-filled row."""
    rows = max(N, 1)
    q = rng.integers(0, 1 << bits, (rows, K)).astype(np.int64) if q is None else q
    scales = oracle.bf16_round(((rng.random((rows, K // 64)) * 0.01 + 0.002) * (255.0 / ((1 << bits) - 1))).astype(np.float32)) if scales is None else scales
    biases = oracle.bf16_round((-rng.random((rows, K // 64))).astype(np.float32)) if biases is None else biases
    a = rng.integers(-3, 4, (M, K)).astype(np.float32) if integer else rng.standard_normal((M, K)).astype(np.float32)
    b = rng.standard_normal((rows,)).astype(np.float32)[:N] if bias else None
    wide = torch.full((M, N + 2 * pad), float("nan"), device="cuda")
    return {"a": torch.from_numpy(a).cuda(), "codes": torch.from_numpy(pack(q, bits)).cuda()[:N], "scales": to_bf16(ltx, scales)[:N],
            "biases": to_bf16(ltx, biases)[:N], "bias": None if b is None else torch.from_numpy(b).cuda(), "in_act": in_act, "wide": wide,
            "out": wide[:, pad:pad + N], "N": N, "K": K, "w": dequant(oracle, q, scales, biases)[:N], "a_np": a, "b_np": b}


def check_jobs(ltx, ctx, jobs, M, bits, **kw):
    ctx.op_gemv_group_q(jobs, bits, M=M, **kw)
    torch.cuda.synchronize()
    for i, j in enumerate(jobs):
        N = j["N"]
        if N:
            want = torch.full((M, N), float("nan"), device="cuda")
            ctx.op_gemv(j["a"], to_bf16(ltx, j["w"]), j["bias"], want, j["in_act"])
            torch.cuda.synchronize()
            assert torch.isfinite(want).all()
            assert torch.equal(j["out"].contiguous().view(torch.int32), want.view(torch.int32)), (i, bits, M, N, j["K"], j["in_act"])
        edge = torch.cat([j["wide"][:, :3], j["wide"][:, 3 + N:]], dim=1)
        assert torch.isnan(edge).all(), f"job {i}: wrote outside its {N} columns"


@pytest.mark.parametrize("bits", [8, 4])
@pytest.mark.parametrize("M", [1, 2, 3, 8])
def test_six_and_eight_jobs_are_each_bit_equal_to_the_gemv_on_the_dequantised_matrix(ltx, oracle, gpu_ctx, bits, M):
    rng = np.random.default_rng(100 * bits + M)
    check_jobs(ltx, gpu_ctx, [make_job(ltx, oracle, rng, bits, M, *s) for s in SIX], M, bits)
    if M in (2, 8):  # eight jobs, the last one empty, once per MMAX instance
        check_jobs(ltx, gpu_ctx, [make_job(ltx, oracle, rng, bits, M, *s) for s in EIGHT], M, bits)


@pytest.mark.parametrize("bits", [8, 4])
@pytest.mark.parametrize("K", [64, 256, 320, 576, 2048, 4096, 4096 + 192])
def test_one_job_per_launch_at_every_chunk_size(ltx, oracle, gpu_ctx, bits, K):
    """n_jobs = 1 (what the ungrouped timestep path launches), N = 3 at M = 2 without and N = 130 at M = 3 with SiLU."""
    rng = np.random.default_rng(bits * 10000 + K)
    check_jobs(ltx, gpu_ctx, [make_job(ltx, oracle, rng, bits, 2, 3, K, 0, True, True)], 2, bits)
    check_jobs(ltx, gpu_ctx, [make_job(ltx, oracle, rng, bits, 3, 130, K, SILU, False, False)], 3, bits)


@pytest.mark.parametrize("bits", [8, 4])
def test_both_scale_bias_routes_give_the_same_bits(ltx, oracle, gpu_ctx, bits):
    """Option "gemvq_sb" = 0 (every lane loads the scale / bias of its group per trip, instead of the default one load per chunk of trips
    + a cross-lane move) against the same reference."""
    rng = np.random.default_rng(7 + bits)
    try:
        gpu_ctx.set_option("gemvq_sb", 0)
        for M in (2, 3):
            check_jobs(ltx, gpu_ctx, [make_job(ltx, oracle, rng, bits, M, *s) for s in SIX], M, bits)
    finally:
        gpu_ctx.set_option("gemvq_sb", 1)


def test_an_empty_job_in_the_middle_is_skipped_and_may_be_null(ltx, oracle, gpu_ctx):
    rng = np.random.default_rng(5)
    jobs = [make_job(ltx, oracle, rng, 8, 3, 130, 256, 0, True, False), make_job(ltx, oracle, rng, 8, 3, 0, 512, SILU, False, False),
            make_job(ltx, oracle, rng, 8, 3, 3, 576, SILU, True, False)]
    check_jobs(ltx, gpu_ctx, jobs, 3, 8)
    for j in (jobs[0], jobs[2]):
        j["wide"].fill_(float("nan"))
    jobs[1].update(a=None, codes=None, scales=None, biases=None, out=None, N=0, K=512)
    check_jobs(ltx, gpu_ctx, jobs, 3, 8)


@pytest.mark.parametrize("bits", [8, 4])
def test_against_float64_on_the_dequantised_weights(ltx, oracle, gpu_ctx, bits):
    """The gemv test's bound: max abs error <= 1e-4 x the reference's max abs, at K = 4096 and 2048 in one launch."""
    rng = np.random.default_rng(3 + bits)
    M = 3
    jobs = [make_job(ltx, oracle, rng, bits, M, N, K, act, True, False) for N, K, act in ((130, 4096, SILU), (1024, 2048, 0), (4, 576, SILU))]
    gpu_ctx.op_gemv_group_q(jobs, bits, M=M)
    torch.cuda.synchronize()
    for j in jobs:
        a = j["a_np"].astype(np.float64)
        a = a / (1 + np.exp(-a)) if j["in_act"] == SILU else a
        want = a @ j["w"].astype(np.float64).T + j["b_np"]
        err, scale = float(np.abs(j["out"].cpu().numpy() - want).max()), float(np.abs(want).max())
        print(f"{bits} bits N={j['N']} K={j['K']}: max abs error against float64 {err:.2e} = {err / scale:.2e} x the reference's max abs {scale:.3f}")
        assert err <= 1e-4 * scale


def test_four_bit_nibble_order(ltx, oracle, gpu_ctx):
    """Even columns +7, odd columns -7 (scale 1, bias -8, codes 15 / 1): a swapped nibble flips every sign. Unit activations on one even
    and one odd column give the two values themselves."""
    rng = np.random.default_rng(11)
    N, K, M = 4, 320, 2
    q = np.where(np.arange(K) % 2 == 0, 15, 1)[None, :].repeat(N, 0).astype(np.int64)
    ones, eights = np.ones((N, K // 64), np.float32), np.full((N, K // 64), -8.0, np.float32)
    j = make_job(ltx, oracle, rng, 4, M, N, K, 0, False, True, q=q, scales=ones, biases=eights)
    a = np.zeros((M, K), np.float32)
    a[0, 70], a[1, 133] = 1.0, 1.0
    j["a"], j["a_np"] = torch.from_numpy(a).cuda(), a
    check_jobs(ltx, gpu_ctx, [j], M, 4)
    out = j["out"].cpu().numpy()
    assert (out[0] == 7.0).all() and (out[1] == -7.0).all(), out


def test_rows_of_a_batch_are_computed_alike(ltx, oracle, gpu_ctx):
    rng = np.random.default_rng(13)
    for M in (2, 8):
        j = make_job(ltx, oracle, rng, 8, M, 130, 4096 + 192, SILU, True, False)
        j["a"] = j["a"][:1].repeat(M, 1).contiguous()
        gpu_ctx.op_gemv_group_q([j], 8, M=M)
        torch.cuda.synchronize()
        for r in range(1, M):
            assert torch.equal(j["out"][0], j["out"][r]), (M, r)


def test_refusals_return_their_status_and_write_nothing(ltx, oracle, gpu_ctx):
    rng = np.random.default_rng(8)

    def fresh(n=2):
        return [make_job(ltx, oracle, rng, 8, 2, 3 + i, 256, 0, True, False) for i in range(n)]

    def refused(jobs, match, bits=8, **kw):
        with pytest.raises(ltx.LTXError, match=match) as e:
            gpu_ctx.op_gemv_group_q(jobs, bits, **kw)
        assert e.value.case == "invalidConfiguration"
        torch.cuda.synchronize()
        for j in jobs:
            assert torch.isnan(j["wide"]).all(), "a refused launch wrote"

    jobs = fresh()
    jobs[1]["K"] = 224  # K % 64 != 0 (the operands are large enough)
    refused(jobs, "job 1", M=2)
    refused(fresh(), "3 bits", bits=3, M=2)
    refused(fresh(), "M=9", M=9)
    refused(fresh(), "M=0", M=0)
    refused(fresh(9), "jobs out of range", M=2)
    refused(fresh(), "jobs out of range", M=2, n_jobs=0)
    for missing in ("a", "codes", "scales", "biases", "out"):
        jobs = fresh()
        jobs[1][missing] = None
        jobs[1]["N"], jobs[1]["K"] = 4, 256
        refused(jobs, "null", M=2)
    check_jobs(ltx, gpu_ctx, fresh(), 2, 8)  # and the same jobs, untouched, run
