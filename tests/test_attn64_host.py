"""CPU tests of the host side of the audio / cross-modal attention: the 1-D position grids, the RoPE tables over real-valued
positions, and the ABI surface of the new entries."""
import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import attn64_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("ltx_audio_positions", "ltx_video_temporal_positions", "ltx_rope_tables_positions", "ltx_attn_module_init_synthetic",
               "ltx_attn_module_load", "ltx_attn_module_unload", "ltx_attn_module_export_param", "ltx_attn_module_forward_dev",
               "ltx_op_attention_hd", "ltx_attention_hd_workgroup_queries", "ltx_op_qknorm_rope_hd")


def test_audio_positions_known_answers_and_helper(ltx):
    p = ltx.audio_positions(3)
    assert p.dtype == np.float32 and np.array_equal(p, np.array([0.005, 0.03, 0.07], np.float32))
    got, want = ltx.audio_positions(126), ref.audio_positions(126)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # frame i >= 1 spans mel frames 4i - 3 .. 4i + 1: middle 4i - 1, times 10 ms
    assert got[125] == np.float32(np.float32(4 * 125 - 1) * np.float32(160) / np.float32(16000))


def test_video_temporal_positions_are_row_0_of_the_position_grid(ltx, oracle):
    for F, H, W in ((2, 2, 3), (4, 16, 24)):
        got = ltx.video_temporal_positions(F, H, W)
        want = oracle.position_grid(F, H, W)[0]
        assert got.shape == (F * H * W,) and np.array_equal(got.view(np.uint32), np.ascontiguousarray(want).view(np.uint32))
    assert np.array_equal(ltx.video_temporal_positions(2, 1, 2, fps=8.0), np.array([0.0625, 0.0625, 0.625, 0.625], np.float32))  # frames [0, 1] and [1, 9] of 8 fps


def test_rope_tables_positions_match_the_f64_helper(ltx):
    """At most 1 ulp of f32 where the C library's cos / sin / pow and Python's differ in the last bit of the f64 result."""
    pos = np.concatenate([ltx.audio_positions(26), ltx.video_temporal_positions(3, 2, 2)])
    for dim in (128, 2048):
        c, s = ltx.rope_tables_positions(pos, dim)
        rc, rs = ref.rope_tables_positions(pos, dim)
        assert c.shape == (pos.size, dim // 2) and c.dtype == np.float32
        assert ref.ulp_distance(c, rc) <= 1 and ref.ulp_distance(s, rs) <= 1
    # position 0.005 s of 20 s -> scaled -0.9995; first frequency pi/2
    import math
    c, s = ltx.rope_tables_positions(np.array([0.005], np.float32), 128)
    ang = (math.pi / 2) * (float(np.float32(0.005)) / 20.0 * 2.0 - 1.0)
    assert abs(float(c[0, 0]) - math.cos(ang)) <= 1e-7 and abs(float(s[0, 0]) - math.sin(ang)) <= 1e-7
    # integer positions over max_pos 4096 are the connector's tables
    c1, s1 = ltx.rope_tables_1d(8, 256)
    c2, s2 = ltx.rope_tables_positions(np.arange(8, dtype=np.float32), 256, max_pos=4096)
    assert np.array_equal(c1, c2) and np.array_equal(s1, s2)


def test_host_entries_reject_bad_arguments(ltx):
    buf = np.zeros(8, np.float32)
    assert ltx.lib.ltx_audio_positions(0, buf.ctypes.data) == 2 and ltx.lib.ltx_audio_positions(4, None) == 2
    assert ltx.lib.ltx_video_temporal_positions(1, 0, 1, 24.0, buf.ctypes.data) == 2
    assert ltx.lib.ltx_rope_tables_positions(buf.ctypes.data, 2, 3, 10000.0, 20, buf.ctypes.data, buf.ctypes.data) == 2
    assert ltx.lib.ltx_attention_hd_workgroup_queries(1, 32, 1536, 128) == 0


def test_workgroup_size_follows_grid_fill(ltx):
    q = ltx.Context.attention_hd_workgroup_queries
    assert q(1, 32, 1536) == 256          # a2v: 6 x 32 = 192 workgroups
    assert q(1, 32, 26) == 64 and q(1, 32, 126) == 64   # audio tokens as queries
    assert q(2, 32, 200) == 128 and q(2, 32, 300) == 256


def test_new_entries_are_declared_exported_bound_and_mirrored(ltx):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ltxhip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(ltx_[a-z0-9_]+)\s*\(", hdr))
    from importlib import import_module

    lib_mod = import_module("ltx-video-swift-mlx_amd._lib")
    so = ctypes.CDLL(lib_mod.SO_PATH)
    for name in NEW_ENTRIES:
        assert name in declared and hasattr(so, name) and name in lib_mod.SIGNATURES, name
    for attr in ("audio_positions", "video_temporal_positions", "rope_tables_positions", "ATTN_QUERY_PRESCALE_64"):
        assert hasattr(ltx, attr), attr
    for attr in ("op_attention_hd", "op_qknorm_rope_hd", "attn_module_init_synthetic", "attn_module_load", "attn_module_unload",
                 "attn_module_export_param", "attn_module_forward_dev", "attention_hd_workgroup_queries"):
        assert hasattr(ltx.Context, attr), attr
    assert np.float32(ltx.ATTN_QUERY_PRESCALE_64) == ref.QUERY_PRESCALE
    assert re.search(r"#define LTX_ABI_VERSION 2\b", open(os.path.join(ROOT, "include", "ltxhip.h")).read())


@pytest.mark.timeout(600)
def test_head_dim_64_attention_kernels_have_no_scratch(tmp_path):
    """Code-object metadata of every attn64_fwd_kernel instance (three workgroup sizes, masked and unmasked): no private segment, no
    spilled registers - the kernel holds up to 192 accumulator / operand registers per lane and a spill would sit inside its key loop.
    Device-side compile only, no GPU needed."""
    import shutil
    import subprocess

    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "ltx-video-swift-mlx_amd", "csrc")
    out = tmp_path / "attention.s"
    subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-S",
                    "--cuda-device-only", "-o", str(out), os.path.join(csrc, "attention.hip")], check=True, capture_output=True)
    kernels = re.findall(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.sgpr_spill_count:\s+(\d+)\n"
                         r"(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)", out.read_text())
    seen = [k for k in kernels if "attn64_fwd_kernel" in k[0]]
    assert len(seen) == 6, [k[0] for k in kernels]
    for name, scratch, sspill, vspill in seen:
        assert int(scratch) == 0 and int(sspill) == 0 and int(vspill) == 0, f"{name}: private segment {scratch} B, spills {sspill} / {vspill}"


# ---- the attention kernel's stress inputs, without a GPU: a numpy replay of the kernel's rounding points (attn64_ref.attention_replay)
# meets, on every input of tests/test_attention_d64_stress_gpu.py, the bounds that file holds the kernel to ----
def test_stress_and_edge_shapes_reach_the_instance_they_name(ltx):
    q = ltx.Context.attention_hd_workgroup_queries
    for instance, shape in ref.INSTANCE_SHAPES.items():
        assert q(*shape) == instance, shape
    for instance, B, H, Tq in ref.EDGE_SHAPES:
        assert q(B, H, Tq) == instance, (B, H, Tq)
    # 128 queries per workgroup are never chosen for Tq <= 128 (the reason EDGE_SHAPES starts that instance at 129)
    assert all(q(B, H, Tq) != 128 for B in (1, 2, 3) for H in range(1, 130) for Tq in (1, 64, 127, 128))


@pytest.mark.parametrize("case", ref.STRESS_CASES + ref.SOFT_BIAS_CASES, ids=ref.case_id)
def test_kernel_replay_meets_the_bounds_on_the_stress_inputs(case):
    builder, args = case
    c = builder(*args)
    want = c.reference()
    got = c.replay()
    err, rel = ref.attention_errors(got, want)
    print(f"{c.name}: replay max abs {err:.3e} rel-L2 {rel:.3e}")
    assert np.isfinite(got).all() and np.isfinite(want).all()
    assert err <= c.bounds[0] and rel <= c.bounds[1], (err, rel)


@pytest.mark.parametrize("case", ref.SOFT_BIAS_CASES, ids=ref.case_id)
@pytest.mark.parametrize("factor", [0.125, 1.4426950408889634], ids=["bias_over_8", "bias_times_log2e"])
def test_soft_bias_in_other_units_is_outside_the_bounds(case, factor):
    """The soft-bias case discriminates: the reference with the bias in a wrong unit misses both bounds."""
    builder, args = case
    c = builder(*args)
    err, rel = ref.attention_errors(c.reference(factor), c.reference())
    print(f"{c.name} bias x {factor}: max abs {err:.3e} rel-L2 {rel:.3e}")
    assert err > c.bounds[0] and rel > c.bounds[1], (err, rel)


def test_soft_bias_at_head_dim_128_discriminates_too():
    c = ref.soft_bias_case(64, False, heads=2, head_dim=128)
    for factor in (1.0 / math.sqrt(128.0), 1.4426950408889634):
        err, rel = ref.attention_errors(c.reference(factor), c.reference())
        assert err > c.bounds[0] and rel > c.bounds[1], (factor, err, rel)


@pytest.mark.parametrize("instance", [64, 128, 256])
def test_masking_the_dominant_key_changes_the_reference(instance):
    """reference_maximum, masked: the two batch elements differ only in the dominant key's bias, and their references differ at its
    query by far more than the bound, so a kernel that ignored the bias there (or applied element 0's to both) cannot pass."""
    c = ref.reference_maximum_case(instance, True)
    want = c.reference()
    row = want[:, ref.DOMINANT_QUERY, :64]
    assert np.abs(row[0] - row[1]).max() > 10 * c.bounds[0]
    plain = ref.reference_maximum_case(instance, False).reference()
    assert np.array_equal(plain[0], plain[1])


def test_one_hot_inputs_select_what_they_promise():
    rng = np.random.default_rng(0)
    for Tk in ref.EDGE_TK:
        q, k, v, sel = ref.one_hot_case(rng, 2, 3, 63, Tk)
        hit = set(sel.ravel().tolist())
        assert {0, Tk - 1} <= hit and set(range(64 * ((Tk - 1) // 64), Tk)) <= hit, Tk
        got = ref.attention_f64(q, k, v, 3, ref.SCALE)
        assert np.abs(got - ref.one_hot_expected(v, sel, 3)).max() <= 1e-3, Tk
