"""dual_step_kernel (csrc/elementwise.hip) through ltx_op_dual_step: CFG, the Euler step and the next forward's bf16 tokens of both
streams of the joint video + audio loop in one launch. The f32 latent, the guided velocity (v_out) and the bf16 tokens must be BIT-EQUAL
to the numpy float32 replay of tests/helpers/dual_denoise_ref.py, in which every operation is one float32 array op: the reference
evaluates the step as separate array ops (LatentUtils.swift:131-141, LTXScheduler.swift:305-327, LTXPipeline.swift:1402), so a fused
multiply-add, an approximate division or the two Euler forms merged into one formula all show in the f32 latent (they do not show in the
bf16 tokens, which is why the latent is compared). Every output sits between canaries."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import dual_denoise_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 16          # canary elements on each side of every output
CANARY = 7.0
SIZES = (4, 8, 1020, 1024, 1028, 128 * 26, 128 * 96, 128 * 1536)  # 128 * 1536 = 192 workgroups' worth: more than one grid pass (128)


def guarded(values, dtype=torch.float32):
    """`values` (1-D numpy, or an element count for an output) between two canary runs, on the device."""
    n = values if isinstance(values, int) else len(values)
    t = torch.full((n + 2 * GUARD,), CANARY, device="cuda", dtype=dtype)
    if not isinstance(values, int):
        t[GUARD:GUARD + n] = torch.from_numpy(values).cuda().to(dtype)
    return t


def inner(t, n):
    return t[GUARD:GUARD + n]


def canaries_intact(t, n):
    return bool((t[:GUARD] == CANARY).all() and (t[GUARD + n:] == CANARY).all())


def make_job(n, form, seed, cfg=None, copies=1, v_out="own"):
    """One job with N(0, 1) operands; v_out: "own" buffer, "alias" (= v_cond) or None."""
    rng = np.random.default_rng(seed)
    h = {"x": rng.standard_normal(n).astype(np.float32), "vc": rng.standard_normal(n).astype(np.float32),
         "vu": rng.standard_normal(n).astype(np.float32) if cfg else None}
    j = {"n": n, "form": form, "cfg_scale": cfg if cfg else 1.0, "copies": copies, "host": h,
         "lat_buf": guarded(h["x"]), "vc_buf": guarded(h["vc"]), "vu_buf": guarded(h["vu"]) if cfg else None,
         "tok_buf": guarded(copies * n, torch.bfloat16)}
    j["vo_buf"] = guarded(n) if v_out == "own" else j["vc_buf"] if v_out == "alias" else None
    j["latent"], j["v_cond"], j["tokens"] = inner(j["lat_buf"], n), inner(j["vc_buf"], n), inner(j["tok_buf"], copies * n)
    j["v_uncond"] = inner(j["vu_buf"], n) if cfg else None
    j["v_out"] = None if j["vo_buf"] is None else inner(j["vo_buf"], n)
    return j


def check(j, sigma, sigma_next):
    """One job's outputs against the replay, bit for bit, and its canaries."""
    n, h = j["n"], j["host"]
    want_x, want_v, want_tok = ref.step(h["x"], h["vc"], h["vu"], j["cfg_scale"], j["form"], sigma, sigma_next)
    got_x = j["latent"].cpu().numpy()
    tag = (n, j["form"], j["cfg_scale"], j["copies"], sigma, sigma_next)
    assert np.array_equal(got_x.view(np.uint32), want_x.view(np.uint32)), ("latent", tag, int((got_x != want_x).sum()))
    tok = j["tokens"].view(torch.int16).cpu().numpy().view(np.uint16).reshape(j["copies"], n)
    for c in range(j["copies"]):
        assert np.array_equal(tok[c], want_tok), ("tokens", c, tag)
    if j["v_out"] is not None:
        got_v = j["v_out"].cpu().numpy()
        assert np.array_equal(got_v.view(np.uint32), want_v.view(np.uint32)), ("v_out", tag)
    for name in ("lat_buf", "vc_buf", "vu_buf", "tok_buf", "vo_buf"):
        if j[name] is not None:
            assert canaries_intact(j[name], j["copies"] * n if name == "tok_buf" else n), (name, tag)
    if j["vo_buf"] is not j["vc_buf"]:  # inputs are read only
        assert np.array_equal(j["v_cond"].cpu().numpy(), h["vc"])


def untouched(j):
    n = j["n"]
    return (np.array_equal(j["latent"].cpu().numpy(), j["host"]["x"]) and bool((j["tokens"] == CANARY).all())
            and (j["vo_buf"] is None or j["vo_buf"] is j["vc_buf"] or bool((j["v_out"] == CANARY).all()))
            and canaries_intact(j["lat_buf"], n) and canaries_intact(j["tok_buf"], j["copies"] * n))


def forms_differ_on_the_cpu(sigma, sigma_next):
    """What makes a swap of the forms (or one formula for both) fail: the replay's two forms differ in at least 10 % of the f32 results
    for N(0, 1) operands at this (sigma, sigma_next > 0). Pure numpy."""
    rng = np.random.default_rng(0)
    x, v = rng.standard_normal(4096).astype(np.float32), rng.standard_normal(4096).astype(np.float32)
    frac = float((ref.euler(x, v, 0, sigma, sigma_next) != ref.euler(x, v, 1, sigma, sigma_next)).mean())
    print(f"sigma {sigma} -> {sigma_next}: the forms differ in {100 * frac:.1f} % of the f32 results")
    assert frac >= 0.10, (sigma, sigma_next, frac)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("sigma,sigma_next", ref.SIGMA_PAIRS)
def test_both_jobs_bit_equal_to_the_float32_replay(gpu_ctx, n, sigma, sigma_next):
    """Video job (form 0, CFG 3.0, two token copies) of n elements and an audio job (form 1, no CFG, one copy) of another size in one
    launch; then the same with CFG and copies exchanged."""
    forms_differ_on_the_cpu(sigma, sigma_next)
    other = SIZES[(SIZES.index(n) + 3) % len(SIZES)]
    for cfg_v, cfg_a, cp_v, cp_a in ((3.0, None, 2, 1), (None, 4.5, 1, 2)):
        jv = make_job(n, 0, seed=n, cfg=cfg_v, copies=cp_v)
        ja = make_job(other, 1, seed=n + 1, cfg=cfg_a, copies=cp_a)
        gpu_ctx.op_dual_step(jv, ja, sigma, sigma_next)
        torch.cuda.synchronize()
        check(jv, sigma, sigma_next)
        check(ja, sigma, sigma_next)


@pytest.mark.parametrize("form", [0, 1])
def test_last_step_sigma_next_zero(gpu_ctx, form):
    jv, ja = make_job(1028, form, seed=5, cfg=3.0, copies=2), make_job(128 * 26, 1 - form, seed=6)
    gpu_ctx.op_dual_step(jv, ja, 0.25, 0.0)
    torch.cuda.synchronize()
    check(jv, 0.25, 0.0)
    check(ja, 0.25, 0.0)


def test_forms_are_not_exchanged(gpu_ctx):
    """The same operands through form 0 and form 1 give the replay's two different latents."""
    sigma, sigma_next = ref.SIGMA_PAIRS[1]
    forms_differ_on_the_cpu(sigma, sigma_next)
    j0, j1 = make_job(4096, 0, seed=9), make_job(4096, 1, seed=9)
    gpu_ctx.op_dual_step(j0, j1, sigma, sigma_next)
    torch.cuda.synchronize()
    check(j0, sigma, sigma_next)
    check(j1, sigma, sigma_next)
    assert float((j0["latent"] != j1["latent"]).float().mean()) >= 0.10


@pytest.mark.parametrize("cfg", [None, 3.0])
def test_v_out_may_alias_v_cond_or_be_absent(gpu_ctx, cfg):
    sigma, sigma_next = ref.SIGMA_PAIRS[2]
    jv, ja = make_job(128 * 96, 0, seed=11, cfg=cfg, v_out="alias"), make_job(1020, 1, seed=12, cfg=cfg, v_out=None)
    gpu_ctx.op_dual_step(jv, ja, sigma, sigma_next)
    torch.cuda.synchronize()
    check(jv, sigma, sigma_next)
    check(ja, sigma, sigma_next)


def test_either_job_may_be_null_or_empty(gpu_ctx):
    sigma, sigma_next = ref.SIGMA_PAIRS[0]
    jv = make_job(1024, 0, seed=13, cfg=3.0)
    gpu_ctx.op_dual_step(jv, None, sigma, sigma_next)
    ja = make_job(1028, 1, seed=14)
    gpu_ctx.op_dual_step(None, ja, sigma, sigma_next)
    jv2, empty = make_job(8, 0, seed=15), make_job(1024, 1, seed=16)
    gpu_ctx.op_dual_step(jv2, dict(empty, n=0), sigma, sigma_next)
    ja2, empty2 = make_job(4, 1, seed=17), make_job(1024, 0, seed=18)
    gpu_ctx.op_dual_step(dict(empty2, n=0), ja2, sigma, sigma_next)
    gpu_ctx.op_dual_step(None, None, sigma, sigma_next)  # nothing to do is not an error
    torch.cuda.synchronize()
    for j in (jv, jv2):
        check(j, sigma, sigma_next)
    for j in (ja, ja2):
        check(j, sigma, sigma_next)
    assert untouched(empty) and untouched(empty2)


def test_bad_arguments_are_refused_before_the_launch(gpu_ctx, ltx):
    """n % 4 != 0, copies outside 1 .. 2, form outside 0 .. 1, a NULL latent / v_cond / tokens, sigma <= 0: invalidConfiguration, and
    neither job's outputs are written."""
    sigma, sigma_next = ref.SIGMA_PAIRS[1]
    good = make_job(1024, 0, seed=21, cfg=3.0, copies=2)
    base = make_job(1024, 1, seed=22, copies=2)
    bads = [dict(base, n=1022), dict(base, copies=0), dict(base, copies=3), dict(base, form=2), dict(base, form=-1), dict(base, latent=None),
            dict(base, v_cond=None), dict(base, tokens=None)]
    for bad in bads:
        for pair in ((good, bad), (bad, good)):
            with pytest.raises(ltx.LTXError) as e:
                gpu_ctx.op_dual_step(pair[0], pair[1], sigma, sigma_next)
            assert e.value.case == "invalidConfiguration", bad
    for s in (0.0, -0.5):
        with pytest.raises(ltx.LTXError, match="sigma") as e:
            gpu_ctx.op_dual_step(good, base, s, 0.0)
        assert e.value.case == "invalidConfiguration"
    torch.cuda.synchronize()
    assert untouched(good) and untouched(base), "a refused call wrote"
