"""CPU checks around the quantised dual model (dual_model_quantize, gemv_group_q_kernel): the new entry points' declarations, exports
and bindings, the code-object numbers of the codes gemv, and its lane -> k -> group -> nibble indexing restated in numpy."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("ltx_dual_model_quantize", "ltx_dual_model_memory_info", "ltx_op_gemv_group_q")


def test_new_entries_are_declared_exported_bound_and_mirrored(ltx):
    hdr_raw = open(os.path.join(ROOT, "include", "ltxhip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr_raw, flags=re.S)
    declared = set(re.findall(r"\b(ltx_[a-z0-9_]+)\s*\(", hdr))
    from importlib import import_module

    lib_mod = import_module("ltx-video-swift-mlx_amd._lib")
    so = ctypes.CDLL(lib_mod.SO_PATH)
    for name in NEW_ENTRIES:
        assert name in declared and hasattr(so, name) and name in lib_mod.SIGNATURES, name
    for attr in ("dual_model_quantize", "dual_model_memory_info", "op_gemv_group_q", "dual_model_load"):
        assert hasattr(ltx.Context, attr), attr
    import inspect

    assert inspect.signature(ltx.Context.dual_model_load).parameters["quant_bits"].default == 16
    assert re.search(r"#define LTX_ABI_VERSION 2\b", hdr_raw)  # additions only: no revision bump
    assert re.search(r"int ltx_dual_model_load\(ltx_ctx\* ctx, const char\* safetensors_path, const ltx_dual_model_config\* cfg\);", hdr)  # untouched
    body = re.search(r"typedef struct ltx_gemv_job_q \{(.*?)\} ltx_gemv_job_q;", hdr, flags=re.S).group(1)
    names = [re.sub(r"\[.*\]", "", d.strip().split()[-1].lstrip("*")) for d in body.split(";") if d.strip()]
    assert names == [f[0] for f in lib_mod.GemvJobQ._fields_], names
    # every new entry cites its reference seam in the header
    for name in NEW_ENTRIES:
        comment = re.findall(r"/\*.*?\*/", hdr_raw[:hdr_raw.index("int " + name + "(")], flags=re.S)[-1]
        assert re.search(r"\.swift:\d+", comment), name
    assert ltx.lib.ltx_dual_model_quantize(None, 8, 64) == 2  # no context: refused, not crashed
    assert ltx.lib.ltx_dual_model_memory_info(None, None, None, None, None) == 2
    assert ltx.lib.ltx_op_gemv_group_q(None, None, 1, 1, 8) == 2


@pytest.mark.timeout(900)
def test_gemv_group_q_kernels_have_no_scratch(tmp_path):
    """Code-object metadata of the gemv_group_q_kernel instances (MMAX 2 / 8 x 8 / 4 bits x both scale / bias routes) for gfx950: no
    private segment and no spilled registers. Device-side compile only, no GPU needed."""
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
    seen = [k for k in kernels if "gemv_group_q_kernel" in k[0]]
    assert len(seen) == 8, [k[0] for k in kernels if "gemv" in k[0]]
    for width in ("Li8ELb", "Li4ELb"):  # both bit widths are there (template arguments <MMAX, BITS, XL>)
        assert sum(width in k[0] for k in seen) == 4, width
    for name, scratch, sspill, vgprs, vspill in seen:
        print(name, "VGPRs", vgprs, "scratch", scratch, "spills", sspill, vspill)
        assert int(scratch) == 0 and int(sspill) == 0 and int(vspill) == 0, f"{name}: private segment {scratch} B, spills {sspill} / {vspill}"
        assert int(vgprs) <= 128


@pytest.mark.parametrize("bits", [8, 4])
@pytest.mark.parametrize("K", [64, 320, 576, 4096 + 192])
def test_lane_to_group_to_nibble_indexing_in_numpy(oracle, bits, K):
    """The kernel's walk restated: trip t, lane l -> k = l * 8 + 512 t (skipped when k >= K); its 8 codes are bytes [k * bits / 8,
    + bits) of the row, element e at bit e * bits of that little-endian word; its group is k >> 6, one scale / bias pair. Summing
    lane partials equals a plain de-quantise (bf16(q * scale + bias)) + matmul (integer operands: every sum is exact)."""
    rng = np.random.default_rng(K + bits)
    N = 3
    q = rng.integers(0, 1 << bits, (N, K))
    scales = rng.integers(1, 4, (N, K // 64)).astype(np.float32)
    biases = -rng.integers(0, 9, (N, K // 64)).astype(np.float32)
    a = rng.integers(-3, 4, (K,)).astype(np.float32)
    packed = q.astype(np.uint8) if bits == 8 else (q[:, 0::2] | (q[:, 1::2] << 4)).astype(np.uint8)
    want = a @ oracle.bf16_round((q.reshape(N, K // 64, 64) * scales[:, :, None] + biases[:, :, None]).astype(np.float32)).reshape(N, K).T
    got = np.zeros(N, np.float32)
    seen = np.zeros(K, bool)
    for n in range(N):
        lanes = np.zeros(64, np.float32)
        for t in range((K + 511) // 512):
            for lane in range(64):
                k = lane * 8 + 512 * t
                if k >= K:
                    continue
                word = int.from_bytes(packed[n, k * bits // 8:k * bits // 8 + bits].tobytes(), "little")
                g = k >> 6
                assert (k + 7) >> 6 == g  # a lane's 8 weights never straddle a group
                for e in range(8):
                    code = (word >> (e * bits)) & ((1 << bits) - 1)
                    lanes[lane] += a[k + e] * oracle.bf16_round(np.array([code * scales[n, g] + biases[n, g]], np.float32))[0]
                    seen[k + e] = True
        got[n] = lanes.sum()
    assert seen.all() and np.array_equal(got, want)
