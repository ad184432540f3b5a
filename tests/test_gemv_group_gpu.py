"""The grouped small-M gemv (gemv_group_kernel, csrc/gemm.hip) through ltx_op_gemv_group: every job of a grouped launch is BIT-EQUAL
to ltx_op_gemv_f32 on the same operands - the same lane -> k mapping, fma chain, wave reduction and bias add, only the weight loads
are issued earlier. Shapes sit where the kernel can go wrong: K = 8 (one lane works), 256 (half a wave), 520 (a partly filled second
trip), 1024 + 512 + 8 (the 2-trip, 1-trip and partial chunks in a row), 2048, 4096 and 4096 + 2048 + 520 (the 8-trip chunk and every
smaller one behind it); N = 1, 5 and 1027 (column tails inside a workgroup and at a job boundary); M = 1, 2, 3, 8 (both MMAX
instances); both activations; a null bias; an N = 0 job in the middle; outputs inside a wider row with a canary around them."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
CANARY = -7.25
SILU = 2
# six jobs of different (N, K, activation, bias) for one launch
SIX = ((5, 8, 0, True), (1027, 256, SILU, True), (1, 520, 0, False), (300, 4096, SILU, True), (64, 1544, 0, True), (13, 6664, SILU, False))


def make_job(gen, M, N, K, in_act, bias, pad=3):
    """Operands of one job; `out` is a view into the middle of a wider canary-filled row ([M][pad + N + pad])."""
    a = torch.randn(M, K, device="cuda", generator=gen)
    W = (torch.randn(max(N, 1), K, device="cuda", generator=gen) / math.sqrt(K)).to(torch.bfloat16)[:N]
    b = torch.randn(max(N, 1), device="cuda", generator=gen)[:N] if bias else None
    wide = torch.full((M, N + 2 * pad), CANARY, device="cuda")
    return {"a": a, "W": W, "bias": b, "in_act": in_act, "wide": wide, "out": wide[:, pad:pad + N], "N": N, "K": K}


def single(ctx, j):
    """ltx_op_gemv_f32 on the job's operands."""
    out = torch.full((j["a"].shape[0], j["N"]), CANARY, device="cuda")
    ctx.op_gemv(j["a"], j["W"], j["bias"], out, j["in_act"])
    return out


def check_jobs(ctx, jobs, M):
    ctx.op_gemv_group(jobs, M=M)
    torch.cuda.synchronize()
    for i, j in enumerate(jobs):
        N = j["N"]
        if N:
            want = single(ctx, j)
            torch.cuda.synchronize()
            assert torch.equal(j["out"].contiguous().view(torch.int32), want.view(torch.int32)), (i, M, N, j["K"], j["in_act"])
            assert torch.isfinite(want).all()
        edge = torch.cat([j["wide"][:, :3], j["wide"][:, 3 + N:]], dim=1)
        assert (edge == CANARY).all(), f"job {i}: wrote outside its {N} columns"


@pytest.mark.parametrize("M", [1, 2, 3, 8])
def test_six_jobs_of_different_shapes_are_each_bit_equal_to_the_single_launch(gpu_ctx, M):
    gen = torch.Generator(device="cuda").manual_seed(10 + M)
    check_jobs(gpu_ctx, [make_job(gen, M, *s) for s in SIX], M)


@pytest.mark.parametrize("K", [8, 256, 520, 2048, 4096])
@pytest.mark.parametrize("in_act", [0, SILU])
def test_one_job_per_launch(gpu_ctx, K, in_act):
    """n_jobs = 1, with N = 5 (a tail inside the last workgroup) at M = 2 and M = 3."""
    gen = torch.Generator(device="cuda").manual_seed(K + in_act)
    for M in (2, 3):
        check_jobs(gpu_ctx, [make_job(gen, M, 5, K, in_act, True)], M)


def test_an_empty_job_in_the_middle_is_skipped(gpu_ctx):
    gen = torch.Generator(device="cuda").manual_seed(5)
    jobs = [make_job(gen, 3, 1027, 256, 0, True), make_job(gen, 3, 0, 512, SILU, False), make_job(gen, 3, 5, 520, SILU, True)]
    check_jobs(gpu_ctx, jobs, 3)
    # the empty job's pointers may be null as well
    for j in (jobs[0], jobs[2]):
        j["wide"].fill_(CANARY)
    jobs[1].update(a=None, W=None, out=None, K=512)
    check_jobs(gpu_ctx, jobs, 3)
    # eight jobs, the first and the last empty
    jobs = [make_job(gen, 2, n, 264, SILU, True) for n in (0, 4, 5, 1, 0, 8, 3, 0)]
    check_jobs(gpu_ctx, jobs, 2)


def test_the_stage_three_layout_of_the_timestep_path(gpu_ctx):
    """A 4-row scale-shift job and a 1-row gate job write one [B][5][D] tensor without a concat pass."""
    gen = torch.Generator(device="cuda").manual_seed(6)
    B, D = 2, 192
    cross = torch.full((B, 5 * D), CANARY, device="cuda")
    h = torch.randn(2, B, D, device="cuda", generator=gen)
    Wss = (torch.randn(4 * D, D, device="cuda", generator=gen) * 0.05).to(torch.bfloat16)
    Wg = (torch.randn(D, D, device="cuda", generator=gen) * 0.05).to(torch.bfloat16)
    bss, bg = torch.randn(4 * D, device="cuda", generator=gen), torch.randn(D, device="cuda", generator=gen)
    gpu_ctx.op_gemv_group([dict(a=h[0], W=Wss, bias=bss, out=cross[:, :4 * D], in_act=SILU),
                           dict(a=h[1], W=Wg, bias=bg, out=cross[:, 4 * D:], in_act=SILU)], M=B)
    ss, gate = torch.empty((B, 4 * D), device="cuda"), torch.empty((B, D), device="cuda")
    gpu_ctx.op_gemv(h[0], Wss, bss, ss, SILU)
    gpu_ctx.op_gemv(h[1], Wg, bg, gate, SILU)
    torch.cuda.synchronize()
    assert torch.equal(cross.view(torch.int32), torch.cat([ss, gate], dim=1).view(torch.int32))


def test_against_float64(gpu_ctx):
    """The tolerance of test_gemv: max abs 1e-4 with W ~ N(0, 1/K), at the real K = 4096 and K = 2048 in one launch."""
    rng = np.random.default_rng(3)
    M, jobs, refs = 3, [], []
    for N, K, in_act in ((300, 4096, SILU), (1027, 2048, 0), (5, 1024, SILU)):
        a = rng.standard_normal((M, K)).astype(np.float32)
        W = torch.from_numpy((rng.standard_normal((N, K)) / math.sqrt(K)).astype(np.float32)).cuda().to(torch.bfloat16)
        bias = rng.standard_normal((N,)).astype(np.float32)
        jobs.append(dict(a=torch.from_numpy(a).cuda(), W=W, bias=torch.from_numpy(bias).cuda(), out=torch.empty((M, N), device="cuda"), in_act=in_act))
        ain = a.astype(np.float64)
        ain = ain / (1 + np.exp(-ain)) if in_act == SILU else ain
        refs.append(ain @ W.float().cpu().numpy().astype(np.float64).T + bias)
    gpu_ctx.op_gemv_group(jobs, M=M)
    torch.cuda.synchronize()
    for j, r in zip(jobs, refs):
        err = np.abs(j["out"].cpu().numpy() - r).max()
        print(f"N={r.shape[1]} K={j['a'].shape[1]}: max abs error against float64 {err:.2e}")
        assert err <= 1e-4


@pytest.mark.parametrize("in_act", [0, SILU])
def test_rows_of_a_batch_are_computed_alike(gpu_ctx, in_act):
    """Identical rows give identical bits, in both MMAX instances (the fma is explicit, as in gemv_f32_kernel)."""
    gen = torch.Generator(device="cuda").manual_seed(7)
    for M in (2, 4, 8):
        jobs = []
        for N, K in ((1027, 256), (301, 4096)):
            j = make_job(gen, M, N, K, in_act, True)
            j["a"] = j["a"][:1].repeat(M, 1).contiguous()
            jobs.append(j)
        gpu_ctx.op_gemv_group(jobs, M=M)
        torch.cuda.synchronize()
        for j in jobs:
            for r in range(1, M):
                assert torch.equal(j["out"][0], j["out"][r]), (M, j["K"], r)


def test_refusals_return_their_status_and_write_nothing(gpu_ctx, ltx):
    gen = torch.Generator(device="cuda").manual_seed(8)

    def fresh():
        return [make_job(gen, 2, 5, 264, 0, True), make_job(gen, 2, 9, 512, SILU, True)]

    def refused(jobs, match, **kw):
        with pytest.raises(ltx.LTXError, match=match) as e:
            gpu_ctx.op_gemv_group(jobs, **kw)
        assert e.value.case == "invalidConfiguration"
        torch.cuda.synchronize()
        for j in jobs:
            assert (j["wide"] == CANARY).all(), "a refused launch wrote"

    refused(fresh(), "jobs out of range", M=2, n_jobs=0)
    refused(fresh(), "jobs out of range", M=2, n_jobs=9)
    refused(fresh(), "M=0", M=0)
    refused(fresh(), "M=9", M=9)
    for bad in (dict(K=260), dict(lda=266), dict(ldw=268), dict(N=-1), dict(K=-8)):  # the alignment rules of ltx_op_gemv_f32, per job
        jobs = fresh()
        jobs[1].update(bad)
        refused(jobs, "job 1", M=2)
    for missing in ("a", "W", "out"):
        jobs = fresh()
        jobs[1][missing] = None
        refused(jobs, "null", M=2)
    check_jobs(gpu_ctx, fresh(), 2)  # and the same jobs, untouched, run
