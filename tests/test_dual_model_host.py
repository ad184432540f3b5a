"""CPU checks around the dual video + audio model (csrc/dual_model.cpp, reference LTX2Transformer.swift:254-392): the condition on
the GPU tests' weights and inputs that makes a GPU pass mean something (every embedder, the timestep each one reads, the place of
the gate row, shift and scale of each head, each caption projection and which context goes where are all visible far outside the
GPU bound), the rounding-point replay's distance from the f32 reference, the checkpoint key map, the new entry points' declarations,
exports and bindings, and the code-object numbers of the grouped gemv kernel."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import dual_model_ref as ref  # noqa: E402

NEW_ENTRIES = ("ltx_op_gemv_group", "ltx_dual_model_config_default", "ltx_dual_model_init_synthetic", "ltx_dual_model_load",
               "ltx_dual_model_unload", "ltx_dual_model_export_param", "ltx_dual_model_forward_dev", "ltx_dual_model_embed_dev")
NARROW = dict(Hv=4, Ha=4, F=2, H=6, W=8, T_a=26, S=70, caption_channels=256)  # the GPU tests' narrow model: 96 video tokens, L = 2
L_NARROW = 2
# the velocities a mistake must move (every one of them by more than 10 x the GPU bound)
AFFECTED = {"drop:adaln_single": ("video",), "drop:audio_adaln_single": ("audio",), "drop:av_ca_video_scale_shift_adaln_single": ("video",),
            "drop:av_ca_a2v_gate_adaln_single": ("video",), "drop:av_ca_audio_scale_shift_adaln_single": ("audio",),
            "drop:av_ca_v2a_gate_adaln_single": ("audio",), "audio_reads_video_timestep": ("audio",), "gate_row_first": ("video", "audio"),
            "swap_head_video": ("video",), "swap_head_audio": ("audio",), "skip_caption_video": ("video",), "skip_caption_audio": ("audio",),
            "swap_contexts": ("video", "audio")}


@pytest.fixture(scope="module", params=[1, 2], ids=["B1", "B2"])
def narrow(request):
    """The f32 reference and the replay, once per batch size; shared by every test below and left unchanged."""
    B = request.param
    w = ref.boost(ref.synth_weights(L_NARROW, NARROW["Hv"], NARROW["Ha"], caption_channels=NARROW["caption_channels"]), NARROW["Hv"], NARROW["Ha"])
    inp = ref.make_inputs(B, seed=B, **NARROW)
    tabs = ref.blocks.tables(None, NARROW["F"], NARROW["H"], NARROW["W"], NARROW["T_a"], NARROW["Hv"], NARROW["Ha"])
    fv, fa = ref.forward(w, L_NARROW, inp, tabs)
    rv, ra = ref.forward(w, L_NARROW, inp, tabs, replay=True)
    return {"w": w, "inp": inp, "tabs": tabs, "f": {"video": fv, "audio": fa}, "replay": {"video": ref.rel_l2(rv, fv), "audio": ref.rel_l2(ra, fa)},
            "replay_cos": {"video": ref.cosine(rv, fv), "audio": ref.cosine(ra, fa)}}


def test_replay_of_the_rounding_points_is_within_the_project_bound(narrow):
    """The numpy replay of the library's rounding points against the f32 reference: what the GPU bound is made from (min(2 x this,
    3e-2)), itself inside the project's module bound."""
    for s in ("video", "audio"):
        print(f"B = {narrow['inp']['B']} {s} velocity: replay vs f32 reference rel-L2 {narrow['replay'][s]:.3e}, cosine {narrow['replay_cos'][s]:.6f}, "
              f"GPU bound {ref.update_bound(narrow['replay'][s]):.3e}")
        assert 1e-4 < narrow["replay"][s] <= 1e-2
        assert narrow["replay_cos"][s] >= 0.9995


@pytest.mark.parametrize("mistake", ref.MISTAKES)
def test_every_piece_is_visible_in_its_velocity(narrow, mistake):
    """Each mistake alone moves the affected velocity by more than ten times the GPU test's bound."""
    mv, ma = ref.forward(narrow["w"], L_NARROW, narrow["inp"], narrow["tabs"], mistake=mistake)
    for s in AFFECTED[mistake]:
        moved = ref.rel_l2(mv if s == "video" else ma, narrow["f"][s])
        bound = ref.update_bound(narrow["replay"][s])
        print(f"{mistake}: {s} velocity moves by {moved:.3e} = {moved / bound:.1f} x bound {bound:.3e}")
        assert moved > 10 * bound, (mistake, s, moved, bound)


def test_unaffected_velocities_do_not_move():
    """The other direction, on a tiny model: a head's swap touches only its own velocity - the mistakes are what their names say."""
    Hv, Ha, L = 1, 1, 1
    w = ref.boost(ref.synth_weights(L, Hv, Ha, seed=3, caption_channels=64), Hv, Ha)
    inp = ref.make_inputs(1, Hv, Ha, 1, 2, 3, 5, 7, caption_channels=64, seed=4)
    fv, fa = ref.forward(w, L, inp)
    sv, sa = ref.forward(w, L, inp, mistake="swap_head_audio")
    assert np.array_equal(sv, fv) and not np.array_equal(sa, fa)
    assert fv.shape == (1, 6, 128) and fa.shape == (1, 5, 128)


def test_embed_rows_and_timesteps():
    """Rows 0-3 of the cross tensors come from the scale-shift embedder and row 4 from the gate embedder; video embedders read the
    video sigma and audio embedders the audio sigma; float64 and f32 agree."""
    Hv, Ha = 1, 1
    w = ref.synth_weights(1, Hv, Ha, seed=2, caption_channels=64)
    inp = ref.make_inputs(2, Hv, Ha, 1, 2, 2, 3, 4, caption_channels=64, seed=1)
    e = ref.embed(w, inp)
    assert e["temb_v"].shape == (2, 6, 128) and e["temb_a"].shape == (2, 6, 64) and e["cross_v"].shape == (2, 5, 128) and e["cross_a"].shape == (2, 5, 64)
    ss, _ = ref.embedder(w, "av_ca_audio_scale_shift_adaln_single", inp["audio_timesteps"])
    gate, _ = ref.embedder(w, "av_ca_v2a_gate_adaln_single", inp["audio_timesteps"])
    assert np.array_equal(e["cross_a"][:, :4].reshape(2, -1), ss) and np.array_equal(e["cross_a"][:, 4], gate)
    wrong, _ = ref.embedder(w, "av_ca_v2a_gate_adaln_single", inp["video_timesteps"])
    assert not np.allclose(gate, wrong, atol=1e-5)
    e64 = ref.embed(w, inp, dtype=np.float64)
    for k in e:
        assert e64[k].dtype == np.float64 and np.abs(e64[k] - e[k]).max() <= 1e-5 * max(1.0, np.abs(e64[k]).max()), k


def test_checkpoint_spelling_round_trips_through_the_documented_key_map():
    keys = ref.param_shapes(2, 1, 1)
    assert len(keys) == 2 * (6 * 10 + 8 + 4) + 2 * 2 + 6 * 6 + 2 * 4 + 2 + 2 * 2
    spelled = {k: ref.checkpoint_spelling(k) for k in keys}
    assert len(set(spelled.values())) == len(keys)
    for k, s in spelled.items():
        assert ref.module_spelling(s) == k, (k, s)
        assert ref.module_spelling(k) == k, k  # the module's own spelling is accepted as it is
    for want in ("proj_in.weight", "time_embed.emb.timestep_embedder.linear_1.weight", "time_embed.linear.bias",
                 "audio_adaln_single.emb.timestep_embedder.linear_2.bias", "av_ca_a2v_gate_adaln_single.emb.timestep_embedder.linear_1.weight",
                 "av_ca_a2v_gate_adaln_single.linear.weight", "audio_patchify_proj.weight", "caption_projection.linear_1.weight",
                 "scale_shift_table", "audio_scale_shift_table", "audio_proj_out.bias", "transformer_blocks.1.audio_ff.net.2.bias"):
        assert want in spelled.values(), want


def test_new_entries_are_declared_exported_bound_and_mirrored(ltx):
    hdr_raw = open(os.path.join(ROOT, "include", "ltxhip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr_raw, flags=re.S)
    declared = set(re.findall(r"\b(ltx_[a-z0-9_]+)\s*\(", hdr))
    from importlib import import_module

    lib_mod = import_module("ltx-video-swift-mlx_amd._lib")
    so = ctypes.CDLL(lib_mod.SO_PATH)
    for name in NEW_ENTRIES:
        assert name in declared and hasattr(so, name) and name in lib_mod.SIGNATURES, name
    for attr in ("dual_model_init_synthetic", "dual_model_load", "dual_model_unload", "dual_model_export_param", "dual_model_forward_dev",
                 "dual_model_embed_dev", "op_gemv_group"):
        assert hasattr(ltx.Context, attr), attr
    assert re.search(r"#define LTX_ABI_VERSION 2\b", hdr_raw)  # additions only: no revision bump
    assert lib_mod.DualModelForwardArgs._fields_[0][0] == "struct_size" and lib_mod.DualModelForwardArgs.struct_size.offset == 0
    for struct, cname in ((lib_mod.DualModelForwardArgs, "ltx_dual_model_forward_args"), (lib_mod.DualModelConfig, "ltx_dual_model_config"),
                          (lib_mod.GemvJob, "ltx_gemv_job")):
        body = re.search(r"typedef struct " + cname + r" \{(.*?)\} " + cname + ";", hdr, flags=re.S).group(1)
        names = []
        for decl in body.split(";"):
            decl = decl.strip()
            if not decl:
                continue
            for part in decl.split(","):
                names.append(re.sub(r"\[.*\]", "", part.strip().split()[-1].lstrip("*")))
        assert names == [f[0] for f in struct._fields_], (cname, names)
    n_init = len(re.search(r"#define LTX_DUAL_MODEL_FORWARD_ARGS_INIT \{(.*?)\}", hdr_raw).group(1).split(","))
    assert n_init == len(lib_mod.DualModelForwardArgs._fields_)
    cfg = ltx.default_dual_model_config()
    assert (cfg.in_channels, cfg.out_channels, cfg.audio_in_channels, cfg.audio_out_channels, cfg.caption_channels) == (128, 128, 128, 128, 3840)
    assert cfg.timestep_scale_multiplier == 1000.0 and (cfg.blocks.num_layers, cfg.blocks.video_dim, cfg.blocks.audio_dim) == (48, 4096, 2048)
    small = ltx.default_dual_model_config(num_layers=2, video_heads=4, audio_heads=4, caption_channels=256)
    assert (small.blocks.video_dim, small.blocks.audio_context_dim, small.caption_channels, small.in_channels) == (512, 256, 256, 128)
    # no context: refused, not crashed
    assert ltx.lib.ltx_dual_model_unload(None) == 2 and ltx.lib.ltx_dual_model_forward_dev(None, None) == 2
    assert ltx.lib.ltx_op_gemv_group(None, None, 1, 1) == 2
    assert ltx.lib.ltx_dual_model_embed_dev(None, None, None, 1, 0, None, None, None, None, None, None) == 2


@pytest.mark.timeout(900)
def test_gemv_group_kernels_have_no_scratch(tmp_path):
    """Code-object metadata of the two gemv_group_kernel instances (MMAX = 2 and 8) for gfx950: no private segment and no spilled
    registers - the eight prefetched weight vectors (32 VGPRs) and the by-value job table stay in registers / the kernarg segment.
    Device-side compile only, no GPU needed."""
    import shutil
    import subprocess

    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "ltx-video-swift-mlx_amd", "csrc")
    out = tmp_path / "gemm.s"
    subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-S",
                    "--cuda-device-only", "-o", str(out), os.path.join(csrc, "gemm.hip")], check=True, capture_output=True)
    kernels = re.findall(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.sgpr_spill_count:\s+(\d+)\n"
                         r"(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)", out.read_text())
    seen = [k for k in kernels if "gemv_group_kernel" in k[0]]
    assert len(seen) == 2, [k[0] for k in kernels if "gemv" in k[0]]
    for name, scratch, sspill, vgprs, vspill in seen:
        print(name, "VGPRs", vgprs, "scratch", scratch, "spills", sspill, vspill)
        assert int(scratch) == 0 and int(sspill) == 0 and int(vspill) == 0, f"{name}: private segment {scratch} B, spills {sspill} / {vspill}"
        assert int(vgprs) <= 128
