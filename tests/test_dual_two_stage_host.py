"""CPU checks around the two-stage video + audio path (csrc/dual_two_stage.h, dual_restage_kernel in csrc/elementwise.hip; reference
LTXPipeline.swift:1613-1817).

(a) the condition on the GPU parity test's inputs that makes its pass mean something: each mistake of dual_two_stage_ref.MISTAKES alone,
    in the f32 reference, moves a final latent by more than 10 x the LARGEST bound that test can use (the upscaler's own error at its
    limit 3e-2). frame0_first cannot show while stage 2 re-noises frame 0 - step 0's re-noise overwrites frame 0 whatever the bridge
    left there - so it is held at the same inputs without the stage-2 draws. The two AdaIN mistakes enter stage 2 through the same door
    as the upscaler's own error, scaled by 1 - sigmas2[0] = 0.09, and reach 5.2 x (skipped) and 9.6 x (statistics exchanged) of that
    largest bound: they are held at 10 x the bound WITHOUT the upscaler allowance, and against the absolute AdaIN bound of
    tests/test_dual_restage_gpu.py (1e-4 on the AdaIN output itself), which they exceed a thousandfold;
(b) the two Euler forms give different f32 stage-2 results, but only by last-place amounts: no parity bound can tell them apart, the
    bit-equality of tests/test_dual_two_stage_gpu.py against a composed form-1 loop is the only guard for the form;
(c) the new entries are declared, exported, bound and mirrored, field for field;
(d) the code object of dual_restage_kernel: no private segment, no spills, the transpose tile its only LDS."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import dual_i2v_ref as iv  # noqa: E402
import dual_model_ref as ref  # noqa: E402
import dual_two_stage_ref as ts  # noqa: E402
import ltx_oracle as oracle  # noqa: E402

AFFECTED = {"adain_skipped": ("video",), "adain_swapped": ("video",), "scales_swapped": ("video",), "audio_not_renoised": ("audio",),
            "audio_noise_planes": ("audio",), "frame0_first": ("video",), "cond_naive": ("video",)}
BELOW_TEN = ("adain_skipped", "adain_swapped")  # module docstring (a)


@pytest.fixture(scope="module")
def narrow():
    """The f32 reference and the rounding-point replay of the whole path at the parity test's setting, once; shared and left unchanged."""
    N = ts.NARROW
    w = ref.boost(ref.synth_weights(ts.L_NARROW, N["Hv"], N["Ha"], caption_channels=N["caption_channels"]), N["Hv"], N["Ha"])
    wu = oracle.synth_upscaler_weights(mid=ts.UPSCALER_MID, seed=ts.UPSCALER_SEED)
    mean, std = ts.vae_stats()
    up = lambda lat: oracle.upsample_latents(wu, lat, mean, std)  # noqa: E731
    case = ts.make_case(steps1=len(ts.SIGMAS1) - 1, steps2=len(ts.SIGMAS2) - 1, seed=1, **N)
    kw = dict(i2v=True, renoise=True, noise_scale=ts.NOISE_SCALE)
    fwd = iv.ref_forward(w, ts.L_NARROW)
    first = ts.stage1(fwd, case, ts.SIGMAS1, **kw)
    f = ts.two_stage(fwd, case, ts.SIGMAS1, ts.SIGMAS2, up, first=first, **kw)
    plain2 = ts.two_stage(fwd, case, ts.SIGMAS1, ts.SIGMAS2, up, first=first, renoise2=False, **kw)
    r = ts.two_stage(iv.ref_forward(w, ts.L_NARROW, replay=True), case, ts.SIGMAS1, ts.SIGMAS2, up, **kw)
    out = {"fwd": fwd, "up": up, "case": case, "kw": kw, "first": first, "f": f, "plain2": plain2, "bound": {}, "replay": {}}
    for k in ("video", "audio"):
        out["replay"][k] = ts.rel_l2(r[k], f[k])
        out["bound"][k], out["allowance"] = ts.parity_bound(out["replay"][k], ts.UPSCALER_BOUND, f["y"], f["z0"], ts.SIGMAS2[0])
    return out


def test_a_replay_of_the_rounding_points_is_small(narrow):
    for k in ("video", "audio"):
        print(f"{k}: replay vs f32 reference rel-L2 {narrow['replay'][k]:.3e}; upscaler allowance at 3e-2 {narrow['allowance']:.3e}; "
              f"largest parity bound {narrow['bound'][k]:.3e}")
        assert 1e-5 < narrow["replay"][k] <= 1e-2
    assert narrow["bound"]["video"] < ts.TWO_STAGE_CAP


@pytest.mark.parametrize("mistake", ts.MISTAKES)
def test_a_every_piece_of_the_bridge_is_visible(narrow, mistake):
    """(a): each mistake alone moves a final latent by more than ten times the parity bound."""
    rn2 = False if mistake == "frame0_first" else None
    want = narrow["plain2"] if mistake == "frame0_first" else narrow["f"]
    got = ts.two_stage(narrow["fwd"], narrow["case"], ts.SIGMAS1, ts.SIGMAS2, narrow["up"], first=narrow["first"], mistake=mistake, renoise2=rn2,
                       **narrow["kw"])
    for k in AFFECTED[mistake]:
        moved = ts.rel_l2(got[k], want[k])
        bound = narrow["bound"][k]
        print(f"{mistake}: {k} latent moves by {moved:.3e} = {moved / bound:.1f} x bound {bound:.3e}")
        if mistake in BELOW_TEN:
            tight = ts.update_bound(narrow["replay"][k])  # the bound a perfect upscaler would leave
            direct = float(np.abs(got["y"] - want["y"]).max())
            print(f"{mistake}: {moved / tight:.1f} x the bound without the upscaler allowance {tight:.3e}; the AdaIN output moves by {direct:.3e} (max abs)")
            assert moved > 10 * tight and moved > bound and direct > 100 * 1e-4, (mistake, k, moved, tight, direct)
        else:
            assert moved > 10 * bound, (mistake, k, moved, bound)
    if mistake == "frame0_first":  # and with the stage-2 draws it cannot show at all
        same = ts.two_stage(narrow["fwd"], narrow["case"], ts.SIGMAS1, ts.SIGMAS2, narrow["up"], first=narrow["first"], mistake=mistake, **narrow["kw"])
        assert np.array_equal(same["video"], narrow["f"]["video"])


def test_b_the_two_euler_forms_differ_by_last_places_only(narrow):
    """(b): stage 2 stepped by the scheduler's form is another f32 result, at a distance no parity bound sees."""
    other = ts.two_stage(narrow["fwd"], narrow["case"], ts.SIGMAS1, ts.SIGMAS2, narrow["up"], first=narrow["first"], video_form2=0, **narrow["kw"])
    f = narrow["f"]
    differ = float(np.mean(other["video"][:, 1:] != f["video"][:, 1:]))
    moved = ts.rel_l2(other["video"], f["video"])
    print(f"form 0 in stage 2: {100 * differ:.1f} % of the stepped f32 results differ, rel-L2 {moved:.3e} (bound {narrow['bound']['video']:.3e})")
    assert differ > 0.05 and moved < 1e-5 < narrow["bound"]["video"]
    assert np.array_equal(other["video"][:, 0:1], f["video"][:, 0:1])  # frame 0 is not stepped


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


def test_c_new_entries_are_declared_exported_bound_and_mirrored(ltx):
    hdr_raw = open(os.path.join(ROOT, "include", "ltxhip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr_raw, flags=re.S)
    from importlib import import_module

    lib_mod = import_module("ltx-video-swift-mlx_amd._lib")
    so = ctypes.CDLL(lib_mod.SO_PATH)
    declared = set(re.findall(r"\b(ltx_[a-z0-9_]+)\s*\(", hdr))
    for name, nargs in (("ltx_op_dual_restage", 3), ("ltx_dual_two_stage_dev", 4), ("ltx_dual_two_stage", 4)):
        assert name in declared and hasattr(so, name) and name in lib_mod.SIGNATURES, name
        assert len(lib_mod.SIGNATURES[name][1]) == nargs
    for attr in ("op_dual_restage", "dual_two_stage_dev", "dual_two_stage"):
        assert hasattr(ltx.Context, attr), attr
    assert re.search(r"#define LTX_ABI_VERSION 2\b", hdr_raw)  # additions only: no revision bump
    for cname, struct in (("ltx_dual_restage_job", lib_mod.DualRestageJob), ("ltx_dual_two_stage_args", lib_mod.DualTwoStageArgs)):
        names = _struct_names(hdr, cname)
        assert names == [f[0] for f in struct._fields_], (cname, names)
    A = lib_mod.DualTwoStageArgs
    assert A._fields_[0][0] == "struct_size" and A.struct_size.offset == 0
    init = [s.strip() for s in re.search(r"#define LTX_DUAL_TWO_STAGE_ARGS_INIT \{(.*?)\}", hdr_raw).group(1).split(",")]
    assert len(init) == len(A._fields_)
    assert init[0] == "(uint32_t)sizeof(ltx_dual_two_stage_args)" and all(v in ("0", "NULL", "0.0f") for v in init[1:])
    assert "cfg_scale" not in [f[0] for f in A._fields_]  # the path is distilled: no CFG field
    # the C++ side mirrors them
    csrc = os.path.join(ROOT, "ltx-video-swift-mlx_amd", "csrc")
    job = re.search(r"struct DualRestageJob \{(.*?)\n\};", open(os.path.join(csrc, "elementwise.h")).read(), flags=re.S).group(1)
    for f in ("x", "latent", "tokens", "C", "T", "noise", "noise_scale", "renoise", "stats", "stats_ref", "HW", "cond", "cond_noise", "cond_scale", "cond_sigma2"):
        assert re.search(r"\b" + f + r" = ", job), f
    dn = re.search(r"struct DualDenoiseParams \{(.*?)\n\};", open(os.path.join(csrc, "dual_denoise.h")).read(), flags=re.S).group(1)
    assert "int video_form = 0;" in dn
    # no context: refused, not crashed
    cb = ltx.PROGRESS_CB(lambda *a: None)
    assert ltx.lib.ltx_op_dual_restage(None, None, None) == 2
    assert ltx.lib.ltx_dual_two_stage_dev(None, None, cb, None) == 2 and ltx.lib.ltx_dual_two_stage(None, None, cb, None) == 2


@pytest.mark.timeout(600)
def test_d_dual_restage_kernel_has_no_scratch(tmp_path):
    """Code-object metadata of dual_restage_kernel for gfx950, by the method of test_dual_step_kernel_has_no_scratch: no private segment,
    no spilled registers, and the 32 x 33 f32 transpose tile (4224 B) as its only LDS. Device-side compile only, no GPU needed."""
    import shutil
    import subprocess

    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "ltx-video-swift-mlx_amd", "csrc")
    out = tmp_path / "elementwise.s"
    subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-S",
                    "--cuda-device-only", "-o", str(out), os.path.join(csrc, "elementwise.hip")], check=True, capture_output=True)
    kernels = re.findall(r"\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n"
                         r"(?:.*\n)*?\s+\.sgpr_spill_count:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)",
                         out.read_text())
    seen = [k for k in kernels if "dual_restage_kernel" in k[1]]
    assert len(seen) == 1, [k[1] for k in kernels]
    lds, name, scratch, sspill, vgprs, vspill = seen[0]
    print(name, "VGPRs", vgprs, "LDS", lds, "scratch", scratch, "spills", sspill, vspill)
    assert int(scratch) == 0 and int(sspill) == 0 and int(vspill) == 0, f"{name}: private segment {scratch} B, spills {sspill} / {vspill}"
    assert int(lds) == 32 * 33 * 4
    assert int(vgprs) <= 64
