"""CPU checks around the dual video + audio transformer block (csrc/dual_block.cpp, reference LTX2TransformerBlock.swift:174-297):
the numpy reference of tests/helpers/dual_block_ref.py against an independent torch restatement; the condition on the GPU tests'
inputs that makes a GPU pass mean something (every one of the eight phases, and the place where normVCA is taken, is visible far
outside the bound); the rounding-point replay's distance from the f32 reference at the GPU tests' narrow shapes; the new entry points'
declarations, exports and bindings; and the code-object numbers of the new row kernel."""
import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import dual_block_ref as ref  # noqa: E402

NEW_ENTRIES = ("ltx_dual_block_config_default", "ltx_dual_blocks_init_synthetic", "ltx_dual_blocks_load", "ltx_dual_blocks_unload",
               "ltx_dual_blocks_export_param", "ltx_dual_blocks_forward_dev", "ltx_op_norm_mod2")
NARROW = dict(Hv=4, Ha=4, F=2, H=6, W=8, T_a=26, S=70)  # the GPU tests' narrow config: 96 video tokens, L = 2
L_NARROW = 2


def _torch_block(w, i, xv, xa, inp, tabs):
    """LTX2TransformerBlock in torch f64, written from the Swift source without the oracle's helpers."""
    import torch

    T = lambda a: torch.from_numpy(np.asarray(a, np.float64))  # noqa: E731
    p = f"transformer_blocks.{i}."
    Hv, Ha = inp["Hv"], inp["Ha"]

    def rms(x, weight=None):
        y = x * torch.rsqrt((x * x).mean(-1, keepdim=True) + 1e-6)
        return y if weight is None else y * weight

    def rope(x, cos, sin, heads):
        b, t, hd = x.shape
        d = hd // heads
        xh = x.view(b, t, heads, 2, d // 2)
        c, s = T(cos)[:t].view(1, t, heads, d // 2), T(sin)[:t].view(1, t, heads, d // 2)
        a, bb = xh[:, :, :, 0], xh[:, :, :, 1]
        return torch.stack([a * c - bb * s, bb * c + a * s], dim=3).reshape(b, t, hd)

    def attn(name, x, heads, context=None, qt=None, kt=None, bias=None):
        g = lambda n: T(w[p + name + n])  # noqa: E731
        ctx = x if context is None else context
        q = rms(x @ g("to_q.weight").T + g("to_q.bias"), g("q_norm.weight"))
        k = rms(ctx @ g("to_k.weight").T + g("to_k.bias"), g("k_norm.weight"))
        v = ctx @ g("to_v.weight").T + g("to_v.bias")
        if qt is not None:
            q, k = rope(q, qt[0], qt[1], heads), rope(k, (kt or qt)[0], (kt or qt)[1], heads)
        b, tq, hd = q.shape
        d = hd // heads
        qh, kh, vh = (t.view(b, -1, heads, d).transpose(1, 2) for t in (q, k, v))
        s = qh @ kh.transpose(-1, -2) / math.sqrt(d)
        if bias is not None:
            s = s + T(bias)[:, None, None, :]
        o = (torch.softmax(s, -1) @ vh).transpose(1, 2).reshape(b, tq, hd)
        return o @ g("to_out.weight").T + g("to_out.bias")

    def ff(name, x):
        h = torch.nn.functional.gelu(x @ T(w[p + name + "project_in.proj.weight"]).T + T(w[p + name + "project_in.proj.bias"]), approximate="tanh")
        return h @ T(w[p + name + "project_out.weight"]).T + T(w[p + name + "project_out.bias"])

    mv = (T(w[p + "scale_shift_table"])[None] + T(inp["temb_video"])).unsqueeze(1)  # [B,1,6,Dv]
    ma = (T(w[p + "audio_scale_shift_table"])[None] + T(inp["temb_audio"])).unsqueeze(1)
    cv = (T(w[p + "scale_shift_table_a2v_ca_video"])[None] + T(inp["cross_video_ss"])).unsqueeze(1)
    ca = (T(w[p + "scale_shift_table_a2v_ca_audio"])[None] + T(inp["cross_audio_ss"])).unsqueeze(1)
    xv = xv + attn("attn1.", rms(xv) * (1 + mv[:, :, 1]) + mv[:, :, 0], Hv, qt=tabs["video"]) * mv[:, :, 2]
    xa = xa + attn("audio_attn1.", rms(xa) * (1 + ma[:, :, 1]) + ma[:, :, 0], Ha, qt=tabs["audio"]) * ma[:, :, 2]
    xv = xv + attn("attn2.", rms(xv), Hv, context=T(inp["context_video"]), bias=inp["bias_video"])
    xa = xa + attn("audio_attn2.", rms(xa), Ha, context=T(inp["context_audio"]), bias=inp["bias_audio"])
    nv, na = rms(xv), rms(xa)
    xv = xv + attn("audio_to_video_attn.", nv * (1 + cv[:, :, 0]) + cv[:, :, 1], Ha, context=na * (1 + ca[:, :, 0]) + ca[:, :, 1],
                   qt=tabs["cross_video"], kt=tabs["cross_audio"]) * cv[:, :, 4]
    xa = xa + attn("video_to_audio_attn.", na * (1 + ca[:, :, 2]) + ca[:, :, 3], Ha, context=nv * (1 + cv[:, :, 2]) + cv[:, :, 3],
                   qt=tabs["cross_audio"], kt=tabs["cross_video"]) * ca[:, :, 4]
    xv = xv + ff("ff.", rms(xv) * (1 + mv[:, :, 4]) + mv[:, :, 3]) * mv[:, :, 5]
    xa = xa + ff("audio_ff.", rms(xa) * (1 + ma[:, :, 4]) + ma[:, :, 3]) * ma[:, :, 5]
    return xv, xa


def test_helper_matches_an_independent_torch_restatement():
    """One tiny case: 1 video head x 128, 2 audio heads x 64, two blocks, (F, H, W) = (2, 2, 3), 5 audio tokens, 7 text tokens, B = 2.
    The only differences are the text K / V roundings to bf16 the helper models (kv_bf16): 2^-9 relative on two operands."""
    import torch

    Hv, Ha, L = 1, 2, 2
    w = ref.synth_weights(L, Hv, Ha, seed=3)
    inp = ref.make_inputs(2, Hv, Ha, 2, 2, 3, 5, 7, seed=4)
    tabs = ref.tables(None, 2, 2, 3, 5, Hv, Ha)
    hv, ha = ref.forward(w, L, inp, tabs)
    xv, xa = torch.from_numpy(inp["x_video"].astype(np.float64)), torch.from_numpy(inp["x_audio"].astype(np.float64))
    for i in range(L):
        xv, xa = _torch_block(w, i, xv, xa, inp, tabs)
    for name, got, want, x in (("video", hv, xv.numpy(), inp["x_video"]), ("audio", ha, xa.numpy(), inp["x_audio"])):
        rel = ref.rel_l2(got - x, want - x)
        print(f"{name}: update rel-L2 helper vs torch f64 = {rel:.3e}")
        assert rel <= 2e-3, (name, rel)   # bf16 K / V of the two text cross-attentions
        assert ref.rel_l2(got, want) <= 5e-4, name


@pytest.fixture(scope="module", params=[1, 2], ids=["B1", "B2"])
def narrow(request):
    B = request.param
    w = ref.synth_weights(L_NARROW, NARROW["Hv"], NARROW["Ha"])
    inp = ref.make_inputs(B, seed=B, **NARROW)
    tabs = ref.tables(None, NARROW["F"], NARROW["H"], NARROW["W"], NARROW["T_a"], NARROW["Hv"], NARROW["Ha"])
    fv, fa = ref.forward(w, L_NARROW, inp, tabs)
    rv, ra = ref.forward(w, L_NARROW, inp, tabs, replay=True)
    upd = {"video": fv - inp["x_video"], "audio": fa - inp["x_audio"]}
    replay = {"video": ref.rel_l2(rv - inp["x_video"], upd["video"]), "audio": ref.rel_l2(ra - inp["x_audio"], upd["audio"])}
    return {"w": w, "inp": inp, "tabs": tabs, "upd": upd, "replay": replay, "stream": {"video": ref.rel_l2(rv, fv), "audio": ref.rel_l2(ra, fa)}}


def test_replay_of_the_rounding_points_at_the_gpu_shapes(narrow):
    """The numpy replay of the library's rounding points against the f32 reference, update and full stream: what the GPU bound is made
    from (update bound = min(2 x this, 3e-2)). The full-width case computes its own on the exported weights (test_dual_block_gpu.py)."""
    for s in ("video", "audio"):
        print(f"B = {narrow['inp']['B']} {s}: replay vs f32 reference, update rel-L2 {narrow['replay'][s]:.3e}, stream rel-L2 {narrow['stream'][s]:.3e}, "
              f"GPU update bound {ref.update_bound(narrow['replay'][s]):.3e}")
        assert 1e-4 < narrow["replay"][s] < 1.5e-2   # bf16 operands: a few 1e-3; the cap of 3e-2 is never what binds here
        assert narrow["stream"][s] <= 1e-2


@pytest.mark.parametrize("phase", ref.PHASES)
def test_every_phase_is_visible_in_its_stream(narrow, phase):
    """Dropping any one phase moves the affected stream's update by at least ten times the GPU bound."""
    s = "video" if phase in ref.VIDEO_PHASES else "audio"
    dv, da = ref.forward(narrow["w"], L_NARROW, narrow["inp"], narrow["tabs"], drop=phase)
    moved = ref.rel_l2((dv if s == "video" else da) - narrow["inp"]["x_" + s], narrow["upd"][s])
    bound = ref.update_bound(narrow["replay"][s])
    print(f"drop {phase}: {s} update moves by {moved:.3e} = {moved / bound:.1f} x bound {bound:.3e}")
    assert moved >= 10 * bound, (phase, moved, bound)


def test_norm_vca_taken_after_the_a2v_update_is_outside_the_bound(narrow):
    dv, da = ref.forward(narrow["w"], L_NARROW, narrow["inp"], narrow["tabs"], norm_vca_after_a2v=True)
    moved = ref.rel_l2(da - narrow["inp"]["x_audio"], narrow["upd"]["audio"])
    bound = ref.update_bound(narrow["replay"]["audio"])
    print(f"late normVCA: audio update moves by {moved:.3e} = {moved / bound:.1f} x bound")
    assert moved > 2 * bound, (moved, bound)


def test_gate_entries_are_of_order_one():
    inp = ref.make_inputs(2, seed=2, **NARROW)
    for t, r in (("temb_video", 2), ("temb_video", 5), ("temb_audio", 2), ("temb_audio", 5), ("cross_video_ss", 4), ("cross_audio_ss", 4)):
        assert 0.3 <= float(np.abs(inp[t][:, r]).mean()) <= 3.0, (t, r)


def test_checkpoint_spelling_round_trip():
    keys = ref.param_shapes(1, 1, 1)
    spelled = {ref.checkpoint_spelling(k) for k in keys}
    assert "transformer_blocks.0.audio_ff.net.0.proj.weight" in spelled and "transformer_blocks.0.ff.net.2.bias" in spelled
    assert "transformer_blocks.0.audio_to_video_attn.to_out.0.weight" in spelled and "transformer_blocks.0.attn1.norm_q.weight" in spelled
    assert "transformer_blocks.0.scale_shift_table_a2v_ca_video" in spelled and len(spelled) == len(keys) == 6 * 10 + 8 + 4


def test_new_entries_are_declared_exported_bound_and_mirrored(ltx):
    hdr_raw = open(os.path.join(ROOT, "include", "ltxhip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr_raw, flags=re.S)
    declared = set(re.findall(r"\b(ltx_[a-z0-9_]+)\s*\(", hdr))
    from importlib import import_module

    lib_mod = import_module("ltx-video-swift-mlx_amd._lib")
    so = ctypes.CDLL(lib_mod.SO_PATH)
    for name in NEW_ENTRIES:
        assert name in declared and hasattr(so, name) and name in lib_mod.SIGNATURES, name
    for attr in ("dual_blocks_init_synthetic", "dual_blocks_load", "dual_blocks_unload", "dual_blocks_export_param", "dual_blocks_forward_dev",
                 "op_norm_mod2"):
        assert hasattr(ltx.Context, attr), attr
    assert re.search(r"#define LTX_ABI_VERSION 2\b", hdr_raw)
    # the size-guarded struct starts with its size; field order of the binding = field order of the header
    assert lib_mod.DualForwardArgs._fields_[0][0] == "struct_size" and lib_mod.DualForwardArgs.struct_size.offset == 0
    for struct, cname in ((lib_mod.DualForwardArgs, "ltx_dual_forward_args"), (lib_mod.DualBlockConfig, "ltx_dual_block_config"),
                          (lib_mod.NormMod2Job, "ltx_norm_mod2_job")):
        body = re.search(r"typedef struct " + cname + r" \{(.*?)\} " + cname + ";", hdr, flags=re.S).group(1)
        names = []
        for decl in body.split(";"):
            decl = decl.strip()
            if not decl:
                continue
            for part in decl.split(","):
                names.append(re.sub(r"\[.*\]", "", part.strip().split()[-1].lstrip("*")))
        assert names == [f[0] for f in struct._fields_], (cname, names)
    cfg = ltx.default_dual_block_config()
    assert (cfg.num_layers, cfg.video_heads, cfg.video_dim, cfg.audio_heads, cfg.audio_dim) == (48, 32, 4096, 32, 2048)
    assert (cfg.video_context_dim, cfg.audio_context_dim, cfg.audio_max_pos, list(cfg.max_pos)) == (4096, 2048, 20, [20, 2048, 2048])
    small = ltx.default_dual_block_config(num_layers=2, video_heads=4, audio_heads=4)
    assert (small.video_dim, small.audio_dim, small.video_context_dim, small.audio_context_dim) == (512, 256, 512, 256)
    # no context: refused, not crashed
    assert ltx.lib.ltx_dual_blocks_unload(None) == 2 and ltx.lib.ltx_dual_blocks_forward_dev(None, None) == 2
    assert ltx.lib.ltx_op_norm_mod2(None, None, None, 1e-6) == 2


@pytest.mark.timeout(600)
def test_norm_mod2_kernels_have_no_scratch(tmp_path):
    """Code-object metadata of the four norm_mod2_kernel instances: no private segment, no spilled registers (the NV = 4 instance holds
    the row and four modulation vectors, 80 registers per lane, across its barrier). Device-side compile only, no GPU needed."""
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
    seen = [k for k in kernels if "norm_mod2_kernel" in k[0]]
    assert len(seen) == 4, [k[0] for k in kernels]
    for name, scratch, sspill, vgprs, vspill in seen:
        print(name, "VGPRs", vgprs, "scratch", scratch, "spills", sspill, vspill)
        assert int(scratch) == 0 and int(sspill) == 0 and int(vspill) == 0, f"{name}: private segment {scratch} B, spills {sspill} / {vspill}"
