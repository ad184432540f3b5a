"""The two kernels image-to-video adds to in the joint video + audio path (csrc/elementwise.hip), through their hooks.

ltx_op_norm_mod2 with a ROW MAP (NormMod2Job::row_map: the modulation row of a video token is row_map[row], per-token timestep groups):
each output must be bit-equal to ltx_op_norm_mod_ex with the same operands and the same map, at every kernel instance (NV = 1, 4 and 2,
8), at the shape where the UNMAPPED ltx_op_norm_mod_ex would take its multi-row kernel, with a map that alternates every row, a map on
one job only and one job NULL.

ltx_op_dual_step with a FROZEN PREFIX (DualStepJob::n_keep / keep_src / keep_noise / keep_scale: frame 0 in token layout): latent, v_out
and the bf16 tokens bit-equal to the numpy float32 replay dual_i2v_ref.step_keep - x' = keep_src + (keep_scale * keep_noise) *
(sigma_next * sigma_next) in four separately rounded operations, or x' = x without noise, v_out and tokens for the whole job - and every
documented refusal writes nothing. Every output sits between canaries."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import dual_i2v_ref as iv  # noqa: E402

pytestmark = pytest.mark.gpu
PAD = 8
GUARD = 16
CANARY = 7.0
FRAME0 = 49152  # H*W*C of one latent frame at 16 x 24 x 128: 48 workgroups' worth; 196608 elements are 192 > the 128 of one grid pass


# ---------------------------------------------------------------------------------------------------------------
# norm_mod2 with a row map
# ---------------------------------------------------------------------------------------------------------------
def make_norm_job(D, rows, G, seed, kind="blocks"):
    """`rows` rows of width D in buffers of row stride D + 8; modulation rows [G][4][D]; a map [rows] of entries in [0, G): "blocks"
    (the image-to-video pattern: the first rows // 2 rows in group 1, the rest in group 0), "alternate" (changes every row) or None."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn((rows, D + PAD), device="cuda", generator=g) * 1.7 + 0.1
    mod = torch.randn((G, 4, D), device="cuda", generator=g) * 0.5
    r = np.arange(rows)
    rm = None if kind is None else ((r < rows // 2).astype(np.int32) if kind == "blocks" else (r % G).astype(np.int32))
    out = lambda: torch.full((rows, D + PAD), CANARY, device="cuda").to(torch.bfloat16)  # noqa: E731
    return {"x": x, "rows": rows, "D": D, "mod": mod, "mod_bstride": 4 * D, "rows_per_batch": max(1, rows // G),
            "scale0": mod[0, 0], "shift0": mod[0, 1], "scale1": mod[0, 2], "shift1": mod[0, 3], "out0": out(), "out1": out(),
            "row_map": None if rm is None else torch.from_numpy(rm).cuda(), "map_host": rm}


def norm_reference(ctx, j):
    outs = []
    for sc, sh in ((j["scale0"], j["shift0"]), (j["scale1"], j["shift1"])):
        o = torch.full((j["rows"], j["D"] + PAD), CANARY, device="cuda").to(torch.bfloat16)
        ctx.op_norm_mod_ex(j["x"], sc, sh, o, j["rows"], j["D"], mod_bstride=j["mod_bstride"], rows_per_batch=j["rows_per_batch"], row_map=j["row_map"])
        outs.append(o)
    return outs


def bf16_bits(t):
    return t.view(torch.int16).cpu().numpy()


def check_norm(ctx, jobs):
    torch.cuda.synchronize()
    for j in jobs:
        want = norm_reference(ctx, j)
        torch.cuda.synchronize()
        for k, w in zip(("out0", "out1"), want):
            assert np.array_equal(bf16_bits(j[k]), bf16_bits(w)), (j["D"], j["rows"], k)  # pad columns included: still the canary
            assert torch.isfinite(j[k][:, :j["D"]].float()).all() and (j[k][:, j["D"]:] == CANARY).all()
        if j["map_host"] is not None and len(set(j["map_host"])) > 1:
            # the map is READ: the unmapped call (row / rows_per_batch) gives other bits on the rows whose group differs
            plain = dict(j, row_map=None, out0=torch.empty_like(j["out0"]), out1=torch.empty_like(j["out1"]))
            ctx.op_norm_mod2(plain, None)
            torch.cuda.synchronize()
            differs = (plain["out0"][:, :j["D"]] != j["out0"][:, :j["D"]]).any(dim=1).cpu().numpy()
            unmapped = np.minimum(np.arange(j["rows"]) // j["rows_per_batch"], j["mod"].shape[0] - 1)
            assert np.array_equal(differs, unmapped != j["map_host"]), (j["D"], j["rows"])


@pytest.mark.parametrize("Dv,rows_v,Da,rows_a", [(512, 96, 256, 26), (4096, 768, 2048, 126), (4100, 10, 256, 26)])
@pytest.mark.parametrize("kind", ["blocks", "alternate"])
def test_norm_mod2_with_a_row_map_is_bit_equal_to_norm_mod_with_the_same_map(gpu_ctx, Dv, rows_v, Da, rows_a, kind):
    """Both jobs mapped, G = 2. (512, 256): NV = 1; (4096, 2048) with 768 / 126 rows: NV = 4 and 2, and 768 rows of D = 4096 is where an
    unmapped ltx_op_norm_mod_ex takes its multi-row kernel; D = 4100: NV = 8, whose modulation vectors are fetched after the reduction."""
    jv, ja = make_norm_job(Dv, rows_v, 2, 1, kind), make_norm_job(Da, rows_a, 2, 2, kind)
    gpu_ctx.op_norm_mod2(jv, ja)
    check_norm(gpu_ctx, (jv, ja))


def test_norm_mod2_map_on_one_job_only_and_one_job_null(gpu_ctx):
    """What the block stack launches: the video job mapped, the audio job by row / rows_per_batch; then each job alone."""
    jv, ja = make_norm_job(512, 96, 2, 3, "blocks"), make_norm_job(256, 26, 2, 4, None)
    gpu_ctx.op_norm_mod2(jv, ja)
    check_norm(gpu_ctx, (jv, ja))
    jv = make_norm_job(4096, 96, 4, 5, "alternate")  # four groups
    gpu_ctx.op_norm_mod2(jv, None)
    check_norm(gpu_ctx, (jv,))
    ja = make_norm_job(2048, 26, 2, 6, "blocks")
    gpu_ctx.op_norm_mod2(None, ja)
    check_norm(gpu_ctx, (ja,))


# ---------------------------------------------------------------------------------------------------------------
# dual_step with a frozen prefix
# ---------------------------------------------------------------------------------------------------------------
def guarded(values, dtype=torch.float32):
    n = values if isinstance(values, int) else len(values)
    t = torch.full((n + 2 * GUARD,), CANARY, device="cuda", dtype=dtype)
    if not isinstance(values, int):
        t[GUARD:GUARD + n] = torch.from_numpy(values).cuda().to(dtype)
    return t


def inner(t, n):
    return t[GUARD:GUARD + n]


def canaries_intact(t, n):
    return bool((t[:GUARD] == CANARY).all() and (t[GUARD + n:] == CANARY).all())


def make_step_job(n, n_keep, seed, form=0, cfg=None, copies=1, noise=True, scale=0.5, new_fields=True):
    rng = np.random.default_rng(seed)
    h = {"x": rng.standard_normal(n).astype(np.float32), "vc": rng.standard_normal(n).astype(np.float32),
         "vu": rng.standard_normal(n).astype(np.float32) if cfg else None,
         "src": rng.standard_normal(n_keep).astype(np.float32), "noise": rng.standard_normal(n_keep).astype(np.float32) if noise else None}
    j = {"n": n, "form": form, "cfg_scale": cfg if cfg else 1.0, "copies": copies, "host": h,
         "lat_buf": guarded(h["x"]), "vc_buf": guarded(h["vc"]), "vu_buf": guarded(h["vu"]) if cfg else None,
         "tok_buf": guarded(copies * n, torch.bfloat16), "vo_buf": guarded(n)}
    j["latent"], j["v_cond"], j["tokens"] = inner(j["lat_buf"], n), inner(j["vc_buf"], n), inner(j["tok_buf"], copies * n)
    j["v_uncond"] = inner(j["vu_buf"], n) if cfg else None
    j["v_out"] = inner(j["vo_buf"], n)
    if new_fields:
        j["n_keep"], j["keep_scale"] = n_keep, scale
        j["keep_src"] = torch.from_numpy(h["src"]).cuda() if n_keep else None
        j["keep_noise"] = torch.from_numpy(h["noise"]).cuda() if (noise and n_keep) else None
    j["expect_keep"] = n_keep
    return j


def check_step(j, sigma, sigma_next):
    n, h = j["n"], j["host"]
    want_x, want_v, want_tok = iv.step_keep(h["x"], h["vc"], h["vu"], j["cfg_scale"], j["form"], sigma, sigma_next, n_keep=j["expect_keep"],
                                            keep_src=h["src"], keep_noise=h["noise"], keep_scale=j.get("keep_scale", 0.0))
    tag = (n, j["expect_keep"], j["form"], j["cfg_scale"], j["copies"], h["noise"] is not None, sigma, sigma_next)
    got_x = j["latent"].cpu().numpy()
    assert np.array_equal(got_x.view(np.uint32), want_x.view(np.uint32)), ("latent", tag, int((got_x != want_x).sum()))
    tok = j["tokens"].view(torch.int16).cpu().numpy().view(np.uint16).reshape(j["copies"], n)
    for c in range(j["copies"]):
        assert np.array_equal(tok[c], want_tok), ("tokens", c, tag)
    got_v = j["v_out"].cpu().numpy()
    assert np.array_equal(got_v.view(np.uint32), want_v.view(np.uint32)), ("v_out", tag)  # the whole job, the prefix included
    for name in ("lat_buf", "vc_buf", "vu_buf", "tok_buf", "vo_buf"):
        if j[name] is not None:
            assert canaries_intact(j[name], j["copies"] * n if name == "tok_buf" else n), (name, tag)
    k = j["expect_keep"]
    if k and h["noise"] is None:
        assert np.array_equal(got_x[:k], h["x"][:k])
    if k and k < n and sigma_next > 0:
        assert not np.array_equal(got_x[k:], h["x"][k:])


def untouched(j):
    n = j["n"]
    return (np.array_equal(j["latent"].cpu().numpy(), j["host"]["x"]) and bool((j["tokens"] == CANARY).all()) and bool((j["v_out"] == CANARY).all())
            and canaries_intact(j["lat_buf"], n) and canaries_intact(j["tok_buf"], j["copies"] * n))


@pytest.mark.parametrize("n,n_keep", [(8, 4), (8, 8), (1024, 0), (4 * FRAME0, FRAME0), (FRAME0 + 4, FRAME0)])
@pytest.mark.parametrize("noise", [True, False])
def test_dual_step_with_a_frozen_prefix_is_bit_equal_to_the_float32_replay(gpu_ctx, n, n_keep, noise):
    """The video job (form 0) with a prefix next to an audio job (form 1) without one, in one launch: without CFG on one token copy, then
    with CFG 3.0 on two; sigma 0.725 -> 0.25. 4 * FRAME0 elements are more than one grid pass; FRAME0 + 4 leaves one vector outside."""
    sigma, sigma_next = 0.725, 0.25
    for cfg, copies in ((None, 1), (3.0, 2)):
        jv = make_step_job(n, n_keep, seed=n + n_keep, cfg=cfg, copies=copies, noise=noise)
        ja = make_step_job(128 * 26, 0, seed=5, form=1, cfg=cfg, copies=copies)
        gpu_ctx.op_dual_step(jv, ja, sigma, sigma_next)
        torch.cuda.synchronize()
        check_step(jv, sigma, sigma_next)
        check_step(ja, sigma, sigma_next)


@pytest.mark.parametrize("noise", [True, False])
def test_dual_step_prefix_on_the_last_step(gpu_ctx, noise):
    """sigma_next = 0: the Euler part ends at the denoised prediction; a re-noised prefix is keep_src + (scale * noise) * 0 = keep_src
    (the loop passes no noise on its last step; the kernel does what it is told)."""
    jv = make_step_job(FRAME0 + 1024, FRAME0, seed=31, cfg=3.0, copies=2, noise=noise)
    gpu_ctx.op_dual_step(jv, None, 0.25, 0.0)
    torch.cuda.synchronize()
    check_step(jv, 0.25, 0.0)
    if noise:
        assert np.array_equal(jv["latent"].cpu().numpy()[:FRAME0], jv["host"]["src"] + np.float32(0) * jv["host"]["noise"])


def test_dual_step_prefix_on_either_job_and_the_audio_form(gpu_ctx):
    """The prefix is a field of the job, not of the video stream: form 1 with a prefix, and both jobs with one."""
    jv, ja = make_step_job(2048, 512, seed=41, form=0, noise=True), make_step_job(1024, 1024, seed=42, form=1, cfg=2.0, noise=True, scale=0.15)
    gpu_ctx.op_dual_step(jv, ja, 0.6, 0.25)
    torch.cuda.synchronize()
    check_step(jv, 0.6, 0.25)
    check_step(ja, 0.6, 0.25)


def test_dual_step_n_keep_zero_equals_a_job_without_the_new_fields(gpu_ctx):
    a = make_step_job(128 * 96, 0, seed=51, cfg=3.0, copies=2)
    b = make_step_job(128 * 96, 0, seed=51, cfg=3.0, copies=2, new_fields=False)
    assert "n_keep" not in b
    gpu_ctx.op_dual_step(a, None, 0.725, 0.25)
    gpu_ctx.op_dual_step(b, None, 0.725, 0.25)
    torch.cuda.synchronize()
    for k in ("lat_buf", "tok_buf", "vo_buf"):
        assert torch.equal(a[k], b[k]), k
    check_step(b, 0.725, 0.25)
    # n_keep = 0 ignores the other prefix fields
    c = make_step_job(128 * 96, 0, seed=51, cfg=3.0, copies=2)
    c["keep_src"], c["keep_noise"], c["keep_scale"] = torch.ones(8, device="cuda"), torch.ones(8, device="cuda"), 3.0
    gpu_ctx.op_dual_step(c, None, 0.725, 0.25)
    torch.cuda.synchronize()
    assert torch.equal(a["lat_buf"], c["lat_buf"]) and torch.equal(a["tok_buf"], c["tok_buf"])


def test_dual_step_prefix_refusals_write_nothing(gpu_ctx, ltx):
    """n_keep % 4 != 0, n_keep < 0, n_keep > n, keep_noise without keep_src: invalidConfiguration before the launch, on either job."""
    good = make_step_job(1024, 256, seed=61, cfg=3.0, copies=2)
    base = make_step_job(1024, 256, seed=62, form=1)
    bads = [dict(base, n_keep=254), dict(base, n_keep=-4), dict(base, n_keep=1028), dict(base, keep_src=None)]
    for bad in bads:
        for pair in ((good, bad), (bad, good)):
            with pytest.raises(ltx.LTXError, match="keep") as e:
                gpu_ctx.op_dual_step(pair[0], pair[1], 0.725, 0.25)
            assert e.value.case == "invalidConfiguration", bad["n_keep"]
    torch.cuda.synchronize()
    assert untouched(good) and untouched(base), "a refused call wrote"
