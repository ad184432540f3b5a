"""Static wait-coverage proof of the generated gfx950 assembly (tools/asm_common.py check_wait_coverage, one checker for the attention
and the GEMM streams): every ds_read of an LDS ring slot is preceded by a vmcnt wait that retires the slot's LDS-DMA fills AND a
barrier; every refill is preceded by an lgkmcnt wait + barrier behind the slot's last reads; a ds_write finds every slot quiet; no
instruction names a register whose LDS read is outstanding. Runs on CPU (no GPU, no assembler): it walks the instruction text.

Background: a prologue that left two staged tiles in flight (`vmcnt(16)`) once passed every parity test and broke run-to-run
repeatability at full size about every second forward. The checker must reject exactly that stream.
"""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEN = os.path.join(ROOT, "tools", "gen_attn_w48.py")
VARIANTS = [[], ["--bias"], ["--prescaled"], ["--bias", "--prescaled"]]
sys.path.insert(0, os.path.join(ROOT, "tools"))
import asm_common as ac  # noqa: E402


@pytest.mark.parametrize("variant", VARIANTS)
def test_attention_stream_is_proven_and_matches_the_committed_file(variant):
    r = subprocess.run([sys.executable, GEN, "--check"] + variant, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "wait coverage ok" in r.stdout and "matches" in r.stdout, r.stdout


@pytest.mark.parametrize("variant", VARIANTS)
def test_checker_rejects_the_prologue_race_that_once_shipped(variant):
    r = subprocess.run([sys.executable, GEN, "--check", "--inject-prologue-race"] + variant, capture_output=True, text=True)
    assert r.returncode != 0
    assert "WaitCoverageError" in r.stderr and "RAW: ds_read of (1, 'K')" in r.stderr, r.stderr[-600:]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("flag,kind", [("--inject-raw-race", "RAW"), ("--inject-war-race", "WAR")])
def test_attention_checker_rejects_injected_races(flag, kind, variant):
    r = subprocess.run([sys.executable, GEN, "--check", flag] + variant, capture_output=True, text=True)
    assert r.returncode != 0 and "WaitCoverageError: " + kind in r.stderr, r.stderr[-400:]


# ---- hand-made streams against a layout in the style of the 48-query attention stream: ring slots of 32 KB (K image, then Vt), slot
# 0 / 1 read through %[ka*], the epilogue's exchange area read back through v56 ----
STAGE = 32768


def _read(addr, off):
    if addr.startswith("%[ka"):
        return off // STAGE, "K"
    return ac.EXCHANGE if addr == "v56" else None


W48 = ac.Layout(lambda m0: (m0 // STAGE, "K" if m0 % STAGE < 16384 else "V"), _read)
FILL = ["s_add_u32 m0, %[wlds], 0", "s_nop 0", "buffer_load_dwordx4 %[ko0], s[36:39], s44 offen lds"]
FILL_V = ["s_add_u32 m0, %[wlds], 16384", "s_nop 0", "buffer_load_dwordx4 %[vo0], s[40:43], s45 offen lds"]
READ = ["ds_read_b128 v[168:171], %[ka0] offset:0"]
STAGED = FILL + ["s_waitcnt vmcnt(0)", "s_barrier"]
LOOP = ["10:"] + READ + ["s_waitcnt lgkmcnt(0)", "s_barrier"] + FILL + ["s_waitcnt vmcnt(0)", "s_barrier", "s_branch 10b"]


def test_checker_rejects_a_refill_without_a_barrier_behind_the_reads():
    """WAR direction, on a hand-made stream: slot 0 is read, then refilled with no barrier in between."""
    assert ac.check_wait_coverage(STAGED + LOOP, W48)["ring_reads"] == 3
    bad = STAGED + ["10:"] + READ + ["s_waitcnt lgkmcnt(0)"] + FILL + ["s_waitcnt vmcnt(0)", "s_barrier", "s_branch 10b"]
    with pytest.raises(ac.WaitCoverageError, match="WAR"):
        ac.check_wait_coverage(bad, W48)
    early = FILL + ["s_barrier", "s_waitcnt vmcnt(0)", "10:"] + READ + ["s_branch 10b"]   # wait AFTER the barrier: not visible
    with pytest.raises(ac.WaitCoverageError, match="RAW"):
        ac.check_wait_coverage(early, W48)


def test_checker_wants_the_ring_quiet_before_a_ds_write():
    """An epilogue that takes the ring area over: its last ring read has returned for this wave (`done`), but only a barrier behind
    that wait says so for the other waves, whose reads the ds_write would overwrite. The write's read-back is an exchange read."""
    tail = ["ds_write_b64 v48, v[60:61] offset:4096", "s_waitcnt lgkmcnt(0)", "ds_read_b128 v[96:99], v56 offset:4096"]
    last = READ + ["s_waitcnt lgkmcnt(0)"]
    assert ac.check_wait_coverage(STAGED + LOOP + last + ["s_barrier"] + tail, W48)["ring_reads"] == 4
    with pytest.raises(ac.WaitCoverageError, match="WAR: ds_write"):
        ac.check_wait_coverage(STAGED + LOOP + last + tail, W48)
    with pytest.raises(ac.WaitCoverageError, match="exchange read"):   # nothing was written to be read back
        ac.check_wait_coverage(STAGED + LOOP + last + ["s_barrier"] + tail[2:], W48)


def test_checker_rejects_an_lds_read_no_mapping_knows():
    with pytest.raises(ac.WaitCoverageError, match="unclassified"):
        ac.check_wait_coverage(STAGED + LOOP + ["ds_read_b128 v[96:99], v77 offset:0"], W48)


@pytest.mark.parametrize("read,consumer", [
    ("ds_read_b128 a[108:111], %[ka0] offset:512", "v_mfma_f32_16x16x32_bf16 v[48:51], a[108:111], v[0:3], v[48:51]"),   # MFMA operand
    ("ds_read_b128 v[184:187], %[ka0]", "v_fma_f32 v48, v186, %[isc], v48"),                                           # VALU consumer
    ("ds_read_b128 a[108:111], %[ka0] offset:512", "ds_read_b128 a[110:113], %[ka1] offset:0"),                          # entry reused
])
def test_checker_rejects_a_register_named_while_its_lds_read_is_outstanding(read, consumer):
    """The newer read keeps the counted wait honest: lgkmcnt(1) covers `read`, lgkmcnt(2) does not."""
    def stream(count):
        return STAGED + LOOP + [read] + READ + [f"s_waitcnt lgkmcnt({count})", consumer, "s_waitcnt lgkmcnt(0)"]
    assert ac.check_wait_coverage(stream(1), W48)["ring_reads"] >= 5
    with pytest.raises(ac.WaitCoverageError, match="REG"):
        ac.check_wait_coverage(stream(2), W48)


def test_a_plain_load_occupies_a_slot_of_the_vmcnt_queue():
    """K of slot 0 is staged, then a plain global_load is issued, then Vt of slot 0; only K is read. The queue is K, load, Vt in issue
    order, so vmcnt(2) retires K: the load takes one of the two slots the wait leaves. A queue of LDS-DMA alone would hold K, Vt and
    retire nothing at that count - which is what the same stream without the load must get; with the load, one more is too many."""
    load = ["global_load_dwordx4 v[0:3], %[qo0], %[qbase] offset:0"]
    reads = ["10:"] + READ + ["s_waitcnt lgkmcnt(0)", "s_branch 10b"]

    def stream(between, count):
        return FILL + between + FILL_V + [f"s_waitcnt vmcnt({count})", "s_barrier"] + reads
    assert ac.check_wait_coverage(stream(load, 2), W48)["ring_fills"] == 2
    with pytest.raises(ac.WaitCoverageError, match=r"RAW: ds_read of \(0, 'K'\)"):
        ac.check_wait_coverage(stream([], 2), W48)
    with pytest.raises(ac.WaitCoverageError, match=r"RAW: ds_read of \(0, 'K'\)"):
        ac.check_wait_coverage(stream(load, 3), W48)


DTL = os.path.join(ROOT, "tools", "gen_gemm_asm_dtl.py")


def test_gemm_192x256_stream_is_proven_and_matches_the_committed_file():
    r = subprocess.run([sys.executable, DTL, "--check"], capture_output=True, text=True)
    assert r.returncode == 0 and "matches" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("flag,kind", [("--inject-raw-race", "RAW"), ("--inject-war-race", "WAR")])
def test_gemm_192x256_checker_rejects_injected_races(flag, kind):
    r = subprocess.run([sys.executable, DTL, "--check", flag], capture_output=True, text=True)
    assert r.returncode != 0 and "WaitCoverageError: " + kind in r.stderr, r.stderr[-400:]


X32 = os.path.join(ROOT, "tools", "gen_attn_x32.py")


def test_attention_x32_stream_is_proven_and_matches_the_committed_file():
    """The 32x32x16 stream keeps fragment reads in flight ACROSS the step barrier and ends every step with vmcnt(0): the proof is
    what says that the reads issued ahead only ever touch slots that were visible one barrier earlier."""
    r = subprocess.run([sys.executable, X32, "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "wait coverage ok" in r.stdout and "matches" in r.stdout, r.stdout


@pytest.mark.parametrize("flag,kind", [("--inject-raw-race", "RAW"), ("--inject-war-race", "WAR")])
def test_attention_x32_checker_rejects_injected_races(flag, kind):
    r = subprocess.run([sys.executable, X32, "--check", flag], capture_output=True, text=True)
    assert r.returncode != 0 and "WaitCoverageError: " + kind in r.stderr, r.stderr[-400:]
