"""CPU checks around the joint video + audio denoise loop (csrc/dual_denoise.cpp, reference LTXPipeline.swift:1276-1417): the condition
on the GPU parity test's inputs that makes its pass mean something (the batch order of the CFG pair, rescale on the video stream only,
the audio context's default and the mask on both streams each move a final latent far outside the GPU bound), the float32 step replay's
own properties, the new entry points' declarations, exports and bindings, and the code-object numbers of dual_step_kernel.

The setting is that of test (h) of tests/test_dual_denoise_gpu.py: narrow boosted model, 3 steps ending at sigma 0, CFG 12, rescale 1.0.
At CFG 3 / rescale 0.7 the random-init model's conditional and unconditional velocities are so close that CFG hardly changes the audio
velocity's spread, and rescaling the audio stream by mistake moves its latent by only 1.5 x the bound; at CFG 12 / 1.0 it moves it by 13 x."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import dual_denoise_ref as dd  # noqa: E402
import dual_model_ref as ref  # noqa: E402

NEW_ENTRIES = ("ltx_op_dual_step", "ltx_dual_model_prepare_text_dev", "ltx_dual_model_text_cache_info", "ltx_dual_denoise_dev", "ltx_dual_denoise")
NARROW = dict(Hv=4, Ha=4, F=2, H=6, W=8, T_a=26, S=70, caption_channels=256)
L_NARROW = 2
SIGMAS = [1.0, 0.725, 0.25, 0.0]
SETTING = dict(cfg_scale=12.0, rescale=1.0)
AFFECTED = {"cfg_order": ("video", "audio"), "rescale_audio": ("audio",), "audio_context_zeros": ("audio",), "mask_one_stream": ("audio",)}


@pytest.fixture(scope="module")
def narrow():
    """The f32 reference loop and the rounding-point replay, once; shared and left unchanged."""
    w = ref.boost(ref.synth_weights(L_NARROW, NARROW["Hv"], NARROW["Ha"], caption_channels=NARROW["caption_channels"]), NARROW["Hv"], NARROW["Ha"])
    case = dd.make_case(cfg=True, seed=1, **NARROW)
    fv, fa, _ = dd.loop(dd.ref_forward(w, L_NARROW), case, SIGMAS, **SETTING)
    rv, ra, _ = dd.loop(dd.ref_forward(w, L_NARROW, replay=True), case, SIGMAS, **SETTING)
    return {"w": w, "case": case, "f": {"video": fv, "audio": fa}, "replay": {"video": dd.rel_l2(rv, fv), "audio": dd.rel_l2(ra, fa)}}


def test_replay_of_the_rounding_points_is_within_the_project_bound(narrow):
    for s in ("video", "audio"):
        print(f"{s} latent after 3 steps: replay vs f32 reference rel-L2 {narrow['replay'][s]:.3e}, GPU bound {dd.update_bound(narrow['replay'][s]):.3e}")
        assert 1e-4 < narrow["replay"][s] <= 1e-2


@pytest.mark.parametrize("mistake", dd.MISTAKES)
def test_every_piece_of_the_loop_is_visible_in_a_final_latent(narrow, mistake):
    """Each mistake alone moves the affected final latent by more than ten times test (h)'s bound."""
    mv, ma, _ = dd.loop(dd.ref_forward(narrow["w"], L_NARROW), narrow["case"], SIGMAS, mistake=mistake, **SETTING)
    for s in AFFECTED[mistake]:
        moved = dd.rel_l2(mv if s == "video" else ma, narrow["f"][s])
        bound = dd.update_bound(narrow["replay"][s])
        print(f"{mistake}: {s} latent moves by {moved:.3e} = {moved / bound:.1f} x bound {bound:.3e}")
        assert moved > 10 * bound, (mistake, s, moved, bound)


def test_the_step_replay_rounds_every_operation_on_its_own():
    """The two Euler forms are different f32 functions (>= 10 % of the results differ at every sigma pair of the GPU tests, while their
    bf16 roundings agree almost everywhere), a fused x - sigma * v differs from the separately rounded one, form 0 ends at the denoised
    prediction when sigma_next = 0, and CFG with scale 1 is the conditional velocity."""
    rng = np.random.default_rng(0)
    x, v, u = (rng.standard_normal(4096).astype(np.float32) for _ in range(3))
    for sigma, sigma_next in dd.SIGMA_PAIRS:
        a, b = dd.euler(x, v, 0, sigma, sigma_next), dd.euler(x, v, 1, sigma, sigma_next)
        frac = float((a != b).mean())
        tok = float((ref.oracle.f32_to_bf16_bits(a) != ref.oracle.f32_to_bf16_bits(b)).mean())
        print(f"sigma {sigma} -> {sigma_next}: forms differ in {100 * frac:.1f} % of the f32 results, {100 * tok:.2f} % of the bf16 tokens")
        assert frac >= 0.10 and tok <= 0.01
        assert np.abs(a - b).max() <= 4 * np.finfo(np.float32).eps * np.abs(a).max()
    s = np.float32(0.725)
    fused = (x.astype(np.float64) - np.float64(s) * v.astype(np.float64)).astype(np.float32)
    assert float((fused != dd.euler(x, v, 0, s, 0.0)).mean()) >= 0.10
    assert np.array_equal(dd.euler(x, v, 0, s, 0.0), x - s * v)
    assert np.array_equal(dd.cfg(v, u, 1.0), v) and np.array_equal(dd.cfg(v, None, 3.0), v)
    y, g, tok = dd.step(x, v, u, 3.0, 1, 0.6, 0.25)
    assert np.array_equal(g, v + np.float32(2.0) * (v - u)) and np.array_equal(tok, ref.oracle.f32_to_bf16_bits(y))


def test_layout_round_trips():
    rng = np.random.default_rng(1)
    v, a = rng.standard_normal((128, 2, 3, 4)).astype(np.float32), rng.standard_normal((8, 5, 16)).astype(np.float32)
    tv, ta = dd.pack_video(v), dd.pack_audio(a)
    assert tv.shape == (24, 128) and ta.shape == (5, 128)
    assert tv[7, 3] == v[3].ravel()[7] and ta[4, 2 * 16 + 5] == a[2, 4, 5]
    assert np.array_equal(dd.unpack_video(tv, 2, 3, 4), v) and np.array_equal(dd.unpack_audio(ta), a)


def test_new_entries_are_declared_exported_bound_and_mirrored(ltx):
    hdr_raw = open(os.path.join(ROOT, "include", "ltxhip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr_raw, flags=re.S)
    declared = set(re.findall(r"\b(ltx_[a-z0-9_]+)\s*\(", hdr))
    from importlib import import_module

    lib_mod = import_module("ltx-video-swift-mlx_amd._lib")
    so = ctypes.CDLL(lib_mod.SO_PATH)
    for name in NEW_ENTRIES:
        assert name in declared and hasattr(so, name) and name in lib_mod.SIGNATURES, name
    for attr in ("op_dual_step", "dual_model_prepare_text", "dual_model_text_cache_info", "dual_denoise_dev", "dual_denoise"):
        assert hasattr(ltx.Context, attr), attr
    assert re.search(r"#define LTX_ABI_VERSION 2\b", hdr_raw)  # additions only: no revision bump
    assert lib_mod.DualDenoiseArgs._fields_[0][0] == "struct_size" and lib_mod.DualDenoiseArgs.struct_size.offset == 0
    for struct, cname in ((lib_mod.DualDenoiseArgs, "ltx_dual_denoise_args"), (lib_mod.DualStepJob, "ltx_dual_step_job")):
        body = re.search(r"typedef struct " + cname + r" \{(.*?)\} " + cname + ";", hdr, flags=re.S).group(1)
        names = []
        for decl in body.split(";"):
            decl = decl.strip()
            if not decl:
                continue
            for part in decl.split(","):
                names.append(re.sub(r"\[.*\]", "", part.strip().split()[-1].lstrip("*")))
        assert names == [f[0] for f in struct._fields_], (cname, names)
    n_init = len(re.search(r"#define LTX_DUAL_DENOISE_ARGS_INIT \{(.*?)\}", hdr_raw).group(1).split(","))
    assert n_init == len(lib_mod.DualDenoiseArgs._fields_)
    assert lib_mod.DualModelForwardArgs._fields_[-1][0] == "text_cache"
    # no context: refused, not crashed
    cb = ltx.PROGRESS_CB(lambda *a: None)
    assert ltx.lib.ltx_op_dual_step(None, None, None, 1.0, 0.5) == 2
    assert ltx.lib.ltx_dual_model_prepare_text_dev(None, None, None, None, None, 1, 1) == 2
    assert ltx.lib.ltx_dual_model_text_cache_info(None, None, None, None, None) == 2
    assert ltx.lib.ltx_dual_denoise_dev(None, None, cb, None) == 2 and ltx.lib.ltx_dual_denoise(None, None, cb, None) == 2


@pytest.mark.timeout(600)
def test_dual_step_kernel_has_no_scratch(tmp_path):
    """Code-object metadata of dual_step_kernel for gfx950: no private segment, no spilled registers; the two by-value jobs stay in the
    kernarg segment. Device-side compile only, no GPU needed."""
    import shutil
    import subprocess

    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "ltx-video-swift-mlx_amd", "csrc")
    out = tmp_path / "elementwise.s"
    subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-S",
                    "--cuda-device-only", "-o", str(out), os.path.join(csrc, "elementwise.hip")], check=True, capture_output=True)
    kernels = re.findall(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.sgpr_spill_count:\s+(\d+)\n"
                         r"(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)", out.read_text())
    seen = [k for k in kernels if "dual_step_kernel" in k[0]]
    assert len(seen) == 1, [k[0] for k in kernels]
    name, scratch, sspill, vgprs, vspill = seen[0]
    print(name, "VGPRs", vgprs, "scratch", scratch, "spills", sspill, vspill)
    assert int(scratch) == 0 and int(sspill) == 0 and int(vspill) == 0, f"{name}: private segment {scratch} B, spills {sspill} / {vspill}"
    assert int(vgprs) <= 64
