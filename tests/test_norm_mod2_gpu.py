"""launch_norm_mod2 (csrc/elementwise.hip) through ltx_op_norm_mod2: the cross-modal norms of the dual block
(LTX2TransformerBlock.swift:246-263) in one launch of two jobs. Each of its two outputs per job must be BIT-EQUAL to the
ltx_op_norm_mod_ex call it replaces (same per-thread sums, wave sums added in wave order), at every width and row count that takes
another kernel instance or launch_norm_mod's multi-row path, with per-batch modulation rows, padded row strides and an empty job."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
PAD = 8


def make_job(D, rows, B, seed, plain1=False):
    """rows = B * rows_per_batch rows of width D in buffers of row stride D + 8; modulation rows [B][4][D] (stride 4 D)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn((rows, D + PAD), device="cuda", generator=g) * 1.7 + 0.1
    mod = torch.randn((B, 4, D), device="cuda", generator=g) * 0.5
    j = {"x": x, "rows": rows, "D": D, "mod": mod, "mod_bstride": 4 * D, "rows_per_batch": rows // B,
         "scale0": mod[0, 0], "shift0": mod[0, 1], "scale1": None if plain1 else mod[0, 2], "shift1": None if plain1 else mod[0, 3],
         "out0": torch.full((rows, D + PAD), 7.0, device="cuda").to(torch.bfloat16), "out1": torch.full((rows, D + PAD), 7.0, device="cuda").to(torch.bfloat16)}
    return j


def reference(ctx, j):
    outs = []
    for sc, sh in ((j["scale0"], j["shift0"]), (j["scale1"], j["shift1"])):
        o = torch.full((j["rows"], j["D"] + PAD), 7.0, device="cuda").to(torch.bfloat16)
        ctx.op_norm_mod_ex(j["x"], sc, sh, o, j["rows"], j["D"], mod_bstride=j["mod_bstride"], rows_per_batch=j["rows_per_batch"])
        outs.append(o)
    return outs


def bits(t):
    return t.view(torch.int16).cpu().numpy()


def check(ctx, jobs):
    for j in jobs:
        if j is None:
            continue
        torch.cuda.synchronize()
        want = reference(ctx, j)
        torch.cuda.synchronize()
        for k, w in zip(("out0", "out1"), want):
            assert np.array_equal(bits(j[k]), bits(w)), (j["D"], j["rows"], k)      # pad columns included: still 7.0
            assert torch.isfinite(j[k][:, :j["D"]].float()).all() and (j[k][:, j["D"]:] == 7.0).all()
            assert not (j[k][:, :j["D"]] == 7.0).all()


@pytest.mark.parametrize("Dv,Da", [(512, 256), (4096, 2048), (2048, 4096), (256, 512)])
@pytest.mark.parametrize("rpb_v,rpb_a", [(1, 26), (97, 1), (26, 97)])
def test_both_outputs_of_both_jobs_are_bit_equal_to_norm_mod(gpu_ctx, Dv, Da, rpb_v, rpb_a):
    """B = 2 with per-batch modulation rows, ldx = ldo = D + 8; D in {256, 512, 2048, 4096} on either job; rows per batch in {1, 26, 97}."""
    B = 2
    jv, ja = make_job(Dv, B * rpb_v, B, 1), make_job(Da, B * rpb_a, B, 2)
    gpu_ctx.op_norm_mod2(jv, ja)
    check(gpu_ctx, (jv, ja))


def test_multi_row_path_of_norm_mod_is_matched(gpu_ctx):
    """D = 4096 with 512+ rows of one batch element: launch_norm_mod takes its R-rows-per-workgroup kernel there; the bits are the same."""
    jv, ja = make_job(4096, 2 * 384, 2, 3), make_job(2048, 2 * 63, 2, 4)
    gpu_ctx.op_norm_mod2(jv, ja)
    check(gpu_ctx, (jv, ja))


def test_one_job_empty_and_a_plain_norm_output(gpu_ctx):
    ja = make_job(256, 26, 1, 5)
    gpu_ctx.op_norm_mod2(None, ja)
    check(gpu_ctx, (ja,))
    jv = make_job(512, 97, 1, 6, plain1=True)   # (scale1, shift1) null: out1 is the plain norm
    empty = make_job(256, 26, 1, 7)
    empty["rows"] = 0
    gpu_ctx.op_norm_mod2(jv, empty)
    check(gpu_ctx, (jv,))
    torch.cuda.synchronize()
    assert (empty["out0"] == 7.0).all() and (empty["out1"] == 7.0).all()
    gpu_ctx.op_norm_mod2(None, None)  # nothing to do is not an error


def test_bad_arguments_are_refused_before_any_write(gpu_ctx, ltx):
    good = make_job(256, 26, 1, 8)
    for change in ({"D": 254}, {"shift0": None}, {"scale1": None}, {"D": 8196}, {"rows": -1}):
        bad = make_job(512, 26, 1, 9)
        bad.update(change)
        with pytest.raises(ltx.LTXError) as e:
            gpu_ctx.op_norm_mod2(good, bad)
        assert e.value.case == "invalidConfiguration", change
        torch.cuda.synchronize()
        for j in (good, bad):
            assert (j["out0"] == 7.0).all() and (j["out1"] == 7.0).all(), change
