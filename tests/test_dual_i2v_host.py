"""CPU checks around image-to-video in the joint video + audio path (per-token video timesteps as timestep groups: csrc/dual_block.h,
csrc/dual_model.h, csrc/dual_denoise.h; reference LTX2Transformer.swift:285-312 and LTXPipeline.swift:1261-1399).

(a) the per-token reference of tests/helpers/dual_i2v_ref.py with one timestep for all tokens IS dual_model_ref.forward, bit for bit;
(b) the new entry point and the appended struct fields are declared, exported, bound and mirrored;
(c) ltx.timestep_groups on hand-made inputs;
(d) the condition on the GPU tests' inputs that makes their pass mean something: each mistake of dual_i2v_ref.MISTAKES alone, on the CPU
    reference, moves a final latent or a velocity by more than 10 x the bound the GPU test uses.

The setting of (d) is that of the parity test of tests/test_dual_i2v_denoise_gpu.py: narrow boosted model (dual_model_ref.boost as it
stands), DISTILLED - 3 steps ending at sigma 0, no CFG - and image_cond_noise_scale 0.5. At CFG 12 / rescale 1.0 (the setting of
tests/test_dual_denoise_host.py) the rounding-point replay, and with it the bound, is five to ten times larger and no mistake but the
Euler step of frame 0 reaches 10 x; at the reference's default noise scale 0.15 the sigma-for-sigma^2 mistake reaches 16 x, at 0.5 it
reaches 50 x. The head's mistake cannot show in a final latent at all - the loop discards the velocity of frame 0, the only tokens whose
head row changes - so it is held against the velocity bound of tests/test_dual_i2v_forward_gpu.py on one forward, at the first step's
sigma; the cross-modal mistake shows in the audio latent (the v2a keys) and in both velocities."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import dual_denoise_ref as dd  # noqa: E402
import dual_i2v_ref as iv  # noqa: E402
import dual_model_ref as ref  # noqa: E402

NARROW = dict(Hv=4, Ha=4, F=2, H=6, W=8, T_a=26, S=70, caption_channels=256)
L_NARROW = 2
SIGMAS = [1.0, 0.725, 0.25, 0.0]
NOISE_SCALE = 0.5
# where each mistake must show: final latents of the loop, or the velocities of one forward
AFFECTED = {"frame0_sigma": ("latent:video", "latent:audio"), "cross_per_batch": ("latent:audio", "velocity:audio"),
            "head_per_batch": ("velocity:video",), "euler_frame0": ("latent:video",), "renoise_sigma": ("latent:video",),
            "renoise_this_sigma": ("latent:video",)}


def narrow_weights():
    return ref.boost(ref.synth_weights(L_NARROW, NARROW["Hv"], NARROW["Ha"], caption_channels=NARROW["caption_channels"]), NARROW["Hv"], NARROW["Ha"])


def forward_inputs(B, sigma, seed=3):
    inp = ref.make_inputs(B, NARROW["Hv"], NARROW["Ha"], NARROW["F"], NARROW["H"], NARROW["W"], NARROW["T_a"], NARROW["S"],
                          caption_channels=NARROW["caption_channels"], seed=seed)
    inp["video_token_timesteps"] = iv.i2v_token_timesteps(B, NARROW["F"], NARROW["H"], NARROW["W"], sigma)
    return inp


@pytest.fixture(scope="module")
def narrow():
    """The f32 reference and the rounding-point replay of the loop and of one forward, once; shared and left unchanged."""
    w = narrow_weights()
    case = dd.make_case(cfg=False, seed=1, **NARROW)
    cond, noise = iv.make_cond(case, len(SIGMAS) - 1)
    kw = dict(noise=noise, noise_scale=NOISE_SCALE)
    fv, fa = iv.loop(iv.ref_forward(w, L_NARROW), case, SIGMAS, cond, **kw)
    rv, ra = iv.loop(iv.ref_forward(w, L_NARROW, replay=True), case, SIGMAS, cond, **kw)
    inp = forward_inputs(1, SIGMAS[0])
    f = iv.forward(w, L_NARROW, inp)
    r = iv.forward(w, L_NARROW, inp, replay=True)
    return {"w": w, "case": case, "cond": cond, "kw": kw, "inp": inp,
            "f": {"latent:video": fv, "latent:audio": fa, "velocity:video": f[0], "velocity:audio": f[1]},
            "replay": {"latent:video": iv.rel_l2(rv, fv), "latent:audio": iv.rel_l2(ra, fa), "velocity:video": iv.rel_l2(r[0], f[0]),
                       "velocity:audio": iv.rel_l2(r[1], f[1])}}


@pytest.mark.parametrize("B", [1, 2])
def test_a_one_timestep_for_all_tokens_is_the_per_batch_reference(B):
    """(a): the per-token tensors [B][T][6][Dv] / [B][T][5][Dv] and the per-token head, with every token at its batch element's
    timestep, give dual_model_ref.forward's velocities exactly - f32 reference and rounding-point replay."""
    w = narrow_weights()
    inp = ref.make_inputs(B, NARROW["Hv"], NARROW["Ha"], NARROW["F"], NARROW["H"], NARROW["W"], NARROW["T_a"], NARROW["S"],
                          caption_channels=NARROW["caption_channels"], seed=3)
    tok = dict(inp)
    tok["video_token_timesteps"] = np.repeat(inp["video_timesteps"][:, None], NARROW["F"] * NARROW["H"] * NARROW["W"], axis=1)
    e = iv.embed_tokens(w, tok)
    assert e["temb_v"].shape == (B, 96, 6, 512) and e["cross_v"].shape == (B, 96, 5, 512) and e["embts_v"].shape == (B, 96, 512)
    for replay in (False, True):
        want = ref.forward(w, L_NARROW, inp, replay=replay)
        got = iv.forward(w, L_NARROW, tok, replay=replay)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), replay
    # and two timesteps are not one: the pin is not vacuous
    tok["video_token_timesteps"] = iv.i2v_token_timesteps(B, NARROW["F"], NARROW["H"], NARROW["W"], inp["video_timesteps"])
    assert not np.array_equal(iv.forward(w, L_NARROW, tok)[1], want[1])


def _struct_names(hdr, cname):
    body = re.search(r"typedef struct " + cname + r" \{(.*?)\} " + cname + ";", hdr, flags=re.S).group(1)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        for part in decl.split(","):
            names.append(re.sub(r"\[.*\]", "", part.strip().split()[-1].lstrip("*")))
    return names


def test_b_new_entry_and_appended_fields_are_declared_exported_bound_and_mirrored(ltx):
    hdr_raw = open(os.path.join(ROOT, "include", "ltxhip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr_raw, flags=re.S)
    from importlib import import_module

    lib_mod = import_module("ltx-video-swift-mlx_amd._lib")
    so = ctypes.CDLL(lib_mod.SO_PATH)
    name = "ltx_dual_model_forward_groups_dev"
    assert name in set(re.findall(r"\b(ltx_[a-z0-9_]+)\s*\(", hdr)) and hasattr(so, name) and name in lib_mod.SIGNATURES
    assert len(lib_mod.SIGNATURES[name][1]) == 4
    for attr in ("dual_model_forward_groups_dev", "dual_model_forward_dev", "dual_blocks_forward_dev", "dual_denoise_dev", "dual_denoise"):
        assert hasattr(ltx.Context, attr), attr
    assert callable(ltx.timestep_groups)
    assert re.search(r"#define LTX_ABI_VERSION 2\b", hdr_raw)  # additions only: no revision bump
    # every struct: the header's fields in the binding's order, the new ones APPENDED after the last field the parent had
    appended = {"ltx_dual_forward_args": (lib_mod.DualForwardArgs, "phase_mask", ["n_groups", "video_row_map"]),
                "ltx_norm_mod2_job": (lib_mod.NormMod2Job, "D", ["row_map"]),
                "ltx_dual_step_job": (lib_mod.DualStepJob, "n", ["n_keep", "keep_src", "keep_noise", "keep_scale"]),
                "ltx_dual_denoise_args": (lib_mod.DualDenoiseArgs, "step_stats", ["cond_latent", "image_cond_noise_scale", "cond_noise"]),
                "ltx_dual_model_forward_args": (lib_mod.DualModelForwardArgs, "text_cache", [])}  # a new function, not new fields
    for cname, (struct, last_old, new) in appended.items():
        names = _struct_names(hdr, cname)
        assert names == [f[0] for f in struct._fields_], (cname, names)
        assert names[names.index(last_old) + 1:] == new, (cname, names)
    for macro, struct in (("LTX_DUAL_FORWARD_ARGS_INIT", lib_mod.DualForwardArgs), ("LTX_DUAL_DENOISE_ARGS_INIT", lib_mod.DualDenoiseArgs),
                          ("LTX_DUAL_MODEL_FORWARD_ARGS_INIT", lib_mod.DualModelForwardArgs)):
        init = re.search(r"#define " + macro + r" \{(.*?)\}", hdr_raw).group(1).split(",")
        assert len(init) == len(struct._fields_), macro
    init = [s.strip() for s in re.search(r"#define LTX_DUAL_FORWARD_ARGS_INIT \{(.*?)\}", hdr_raw).group(1).split(",")]
    assert init[[f[0] for f in lib_mod.DualForwardArgs._fields_].index("n_groups")] == "1"  # the default is one group
    # the C++ side mirrors them too
    ew = open(os.path.join(ROOT, "ltx-video-swift-mlx_amd", "csrc", "elementwise.h")).read()
    job = re.search(r"struct NormMod2Job \{(.*?)\n\};", ew, flags=re.S).group(1)
    assert re.search(r"const int32_t\* row_map = nullptr;", job)
    step = re.search(r"struct DualStepJob \{(.*?)\n\};", ew, flags=re.S).group(1)
    for decl in ("long n_keep = 0;", "const float* keep_src = nullptr;", "const float* keep_noise = nullptr;", "float keep_scale = 0.0f;"):
        assert decl in step, decl
    # no context: refused, not crashed
    assert ltx.lib.ltx_dual_model_forward_groups_dev(None, None, 2, None) == 2


def test_c_timestep_groups(ltx):
    """(c): distinct values per batch element in order of first appearance; row_map[b*T + t] = b*G + group; padding repeats the first
    value; more than 8 rows in all is refused."""
    ts, rm = ltx.timestep_groups(np.asarray([[0.0, 0.0, 0.75, 0.75, 0.75]], np.float32))
    assert ts.dtype == np.float32 and rm.dtype == np.int32
    assert np.array_equal(ts, [[0.0, 0.75]]) and np.array_equal(rm, [0, 0, 1, 1, 1])
    ts, rm = ltx.timestep_groups(np.asarray([[0.5, 0.5, 0.5], [0.25, 0.0, 0.25]], np.float32))
    assert np.array_equal(ts, np.asarray([[0.5, 0.5], [0.25, 0.0]], np.float32)) and np.array_equal(rm, [0, 0, 0, 2, 3, 2])
    ts, rm = ltx.timestep_groups(np.asarray([[0.9, 0.1, 0.9, 0.3, 0.1, 0.3]], np.float32))  # interleaved, three groups
    assert np.array_equal(ts, np.asarray([[0.9, 0.1, 0.3]], np.float32)) and np.array_equal(rm, [0, 1, 0, 2, 1, 2])
    ts, rm = ltx.timestep_groups(np.full((2, 4), 0.6, np.float32))                          # one group: the per-batch form
    assert ts.shape == (2, 1) and np.array_equal(rm, [0, 0, 0, 0, 1, 1, 1, 1])
    ts, rm = ltx.timestep_groups(np.arange(8, dtype=np.float32)[None] / 8)                    # exactly 8 rows pass
    assert ts.shape == (1, 8) and np.array_equal(rm, np.arange(8))
    # the helper's own restatement agrees, on the image-to-video pattern too
    tt = iv.i2v_token_timesteps(2, 2, 6, 8, [0.7, 0.3])
    vals, grp = iv.timestep_groups(tt)
    ts, rm = ltx.timestep_groups(tt)
    assert np.array_equal(ts, vals) and np.array_equal(rm.reshape(2, -1), grp + np.asarray([[0], [2]]))
    assert np.array_equal(ts.reshape(-1)[rm].reshape(2, -1), tt)  # the map picks every token's own timestep
    with pytest.raises(ValueError, match="distinct"):
        ltx.timestep_groups(np.arange(9, dtype=np.float32)[None] / 9)                         # 9 distinct values
    with pytest.raises(ValueError, match="distinct"):
        ltx.timestep_groups(np.asarray([[0.1, 0.2, 0.3, 0.4, 0.5]] * 2, np.float32))          # B * G = 10
    with pytest.raises(ValueError):
        ltx.timestep_groups(np.zeros(5, np.float32))


def test_d_replay_of_the_rounding_points_is_within_the_project_bound(narrow):
    for k, rep in narrow["replay"].items():
        print(f"{k}: replay vs f32 reference rel-L2 {rep:.3e}, GPU bound {iv.update_bound(rep):.3e}")
        assert 1e-4 < rep <= 1e-2


def test_d_frame0_of_the_reference_is_the_last_noised_frame(narrow):
    """What the GPU loop must reproduce: frame 0 after the loop is cond + (scale * noise[last]) * sigma_last^2 with the LAST step's sigma
    (the reference re-noises only at the start of a step), and cond itself without noise; the step launch's frozen prefix, which writes
    frame 0 for the NEXT step at the end of a step, gives the same values."""
    fv = narrow["f"]["latent:video"]
    noise = narrow["kw"]["noise"]
    s = np.float32(SIGMAS[-2])
    assert np.array_equal(fv[:, 0:1], iv.noised(narrow["cond"], noise[-1], NOISE_SCALE, np.float32(s * s)))
    plain, _ = iv.loop(lambda inp: (np.zeros((1, 96, 128), np.float32), np.zeros((1, 26, 128), np.float32)), narrow["case"], SIGMAS, narrow["cond"])
    assert np.array_equal(plain[:, 0:1], narrow["cond"])
    rng = np.random.default_rng(0)
    x, v, c, z = (rng.standard_normal(64).astype(np.float32) for _ in range(4))
    y, g, tok = iv.step_keep(x, v, None, 1.0, 0, 0.725, 0.25, n_keep=16, keep_src=c, keep_noise=z, keep_scale=NOISE_SCALE)
    assert np.array_equal(y[:16], iv.noised(c[:16], z[:16], NOISE_SCALE, np.float32(np.float32(0.25) * np.float32(0.25))))
    assert np.array_equal(y[16:], dd.euler(x, v, 0, 0.725, 0.25)[16:]) and np.array_equal(g, v) and np.array_equal(tok, ref.oracle.f32_to_bf16_bits(y))
    y, _, _ = iv.step_keep(x, v, None, 1.0, 0, 0.725, 0.25, n_keep=16)
    assert np.array_equal(y[:16], x[:16])


@pytest.mark.parametrize("mistake", iv.MISTAKES)
def test_d_every_piece_of_image_to_video_is_visible(narrow, mistake):
    """(d): each mistake alone moves a final latent of the loop, or a velocity of one forward, by more than ten times the GPU bound."""
    w = narrow["w"]
    got = {}
    if any(k.startswith("latent") for k in AFFECTED[mistake]):
        if mistake in iv.MODEL_MISTAKES:
            mv, ma = iv.loop(iv.ref_forward(w, L_NARROW, mistake=mistake), narrow["case"], SIGMAS, narrow["cond"], **narrow["kw"])
        else:
            mv, ma = iv.loop(iv.ref_forward(w, L_NARROW), narrow["case"], SIGMAS, narrow["cond"], mistake=mistake, **narrow["kw"])
        got.update({"latent:video": mv, "latent:audio": ma})
    if any(k.startswith("velocity") for k in AFFECTED[mistake]):
        g = iv.forward(w, L_NARROW, narrow["inp"], mistake=mistake)
        got.update({"velocity:video": g[0], "velocity:audio": g[1]})
    for k in AFFECTED[mistake]:
        moved = iv.rel_l2(got[k], narrow["f"][k])
        bound = iv.update_bound(narrow["replay"][k])
        print(f"{mistake}: {k} moves by {moved:.3e} = {moved / bound:.1f} x bound {bound:.3e}")
        assert moved > 10 * bound, (mistake, k, moved, bound)
