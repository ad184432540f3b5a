#!/usr/bin/env python3
"""Generates ltx-video-swift-mlx_amd/csrc/gemm_tall_384x256.inc (+ _clobbers.inc, _dump.inc): the gfx950 assembly main loop of
gemm_bf16_kernel_tall (gemm_asm_tiles.inc, tile_cfg 76). The generated files are committed; the build does not run this script. Sibling of
tools/gen_gemm_asm_dtl.py (the 192 x 256 stream) and tools/gen_gemm_asm_qkv.py (192 x 384), whose outputs this script never touches.

C[M][N] = A[M][K] . B[N][K]^T, bf16 in, f32 accumulate. Workgroup tile 384 x 256: the DiT's FFN-up projection at 1536 tokens
(1536 x 16384) is exactly ONE round of 4 x 64 = 256 such tiles where 192 x 256 tiles need two. Four waves as 2 x 2 = ONE wave per SIMD,
wave tile 192 x 128 = 12 x 8 accumulators of v_mfma_f32_16x16x32_bf16, K-tiles of 64, the LDS image of every other GEMM kernel of this
library (128-byte rows, 16-byte chunks XOR-swizzled by (row >> 1) & 7 on the LDS-DMA source address, 8-row pieces of 1 KB per wave
instruction). Per MFMA the tile stages (384 + 256) / (384 * 256) bytes against (192 + 256) / (192 * 256): 29 % fewer, 20 fragment reads
per 96 MFMAs instead of 28, 20 LDS-DMA pieces per 192 MFMAs per wave instead of 28.

Structure (a 48 + 32 KB K-tile: TWO slots for the activations and TWO for the weights are the whole 160 KB of LDS, so the kernel has no
static LDS and the epilogue reuses the slots):
  * the 8 B fragments of BOTH k-steps of a K-tile are held in registers (64 VGPRs); the 12 A fragments of a k-step stream through a
    ring of RING x 4 VGPRs: with the row fragment as the outer MFMA loop each A fragment feeds 8 consecutive MFMAs, and its ring slot is
    reloaded RING - 1 fragments (~ 370 cycles) ahead of its first use;
  * per K-tile t (A slot t % 2, B slot t % 2), 192 MFMAs per wave, in one in-order stream (default positions):
      MFMA   1..8    one ds_read of a k-step-1 B fragment behind each; the rest of the LDS-DMA pieces of A(t+1) -> A slot (t+1) % 2
      after BAR1     counted lgkmcnt + s_barrier     every wave holds both k-steps' B fragments: B slot t % 2 is free          [WAR]
      then           8 LDS-DMA pieces of B(t+2) -> B slot t % 2 (weights are the HBM-cold operand: requested 1.9 tiles ahead)
      after BAR2     s_waitcnt vmcnt(8) lgkmcnt(0) + s_barrier   A(t+1), B(t+1) have landed, only B(t+2) may fly               [RAW]
                     ... and every wave's last A read of tile t has returned: A slot t % 2 is free                            [WAR]
      MFMA 169..192  the reads of tile t+1's k-step-0 B fragments and first A fragments; the first ATAIL pieces of A(t+2)
    A(t+1) is always issued before B(t+2), so the counted wait leaves exactly the 8 newer weight pieces in flight. Two barriers and
    no VALU instruction per K-tile; the loop body is two tiles long, left after either. Every wait is derived from the issue order;
    check_wait_coverage() (tools/asm_common.py, shared with every proven stream) proves both hazards and the operand waits,
    check_products() the operand of every MFMA on the emitted text before it is written.
  * one accumulator chain per output element, K ascending, A = activations, B = weights: bit-identical to the 192 x 256 stream and to
    the 192 x 128 ring kernel on the same operands.

Register map (per wave):
  v[0:31] / v[32:63]  B fragments of k-step 0 / 1          v[64:79]  A ring
  a[0:255]    accumulators of row fragments 0..7, a[(mi*8 + ni)*4 ..]: the map of the 192 x 256 stream extended by one 32-row group
  v[80:207]   accumulators of row fragments 8..11 (384 accumulator registers do not fit 256 AGPRs). The C++ epilogue behind the asm
              block cannot see clobbered VGPRs, so the stream ends by writing them to LDS in the layout of the epilogue's scratch
              ([sp] + 16 KB per 32-row group, behind a barrier: every wave's LDS-DMA has landed, no slot is read any more).
  v[208:209] / v[210:211] fragment addresses of A / B slot 1
  s[36:39] / s[40:43] A / B buffer descriptors   s46 tile counter   s[50:61] / s[62:69] scalar offsets of the A / B pieces
"""
import os
import re
import sys

from asm_common import Stream, WaitCoverageError, check_wait_coverage, clobbers_inc, emit, finish, knobs, read_slot_from, slot_layout, vr, walk

MI, NI = 12, 8
MI_AGPR = 8                   # row fragments 0..7 accumulate in AGPRs, 8..11 in VGPRs
NA, NB = 12, 8                # LDS-DMA pieces per wave and K-tile
A_BYTES = 384 * 128           # 49152 per A slot
B_BYTES = 256 * 128           # 32768 per B slot
A_SLOTS, B_SLOTS = 2, 2       # LDS: [A0][A1][B0][B1] = 163840 bytes
BSET = (0, 32)                # B fragments of the two k-steps
ARING = 64
VACC = 80
S1 = 208                      # fragment addresses of slot 1: A k-step 0 / 1, B k-step 0 / 1
NV = S1 + 4
SA, SB = 50, 62               # first scalar offset of the A / B pieces
STAMP0, SAVE_M0 = 70, 86
NM = 2 * MI * NI              # MFMAs per K-tile
RING = 4
B1_FIRST, B1_EVERY = 1, 1     # k-step-1 B reads of this tile
BAR1_AFTER = 16
ATAIL = 4                     # pieces of A(t+2) issued behind BAR2 of tile t; the others at the start of tile t+1
ADMA_FIRST, ADMA_EVERY = 2, 3
BDMA_FIRST, BDMA_EVERY = 26, 4
BAR2_AFTER = 168
NEXT_FIRST, NEXT_EVERY = 169, 2
TDMA_FIRST, TDMA_EVERY = 170, 6
STAMPS = "--stamps" in sys.argv   # diagnostic build (tools/ubench/gemm_tall_stamps.hip): s_memtime at the phase boundaries of body 0
# schedule knobs for A/B builds: TALL_KNOBS="ring=4,bar1=16,atail=4,adma0=2,admae=3,bdma0=26,bdmae=4,bar2=168,next=169,nexte=2,tdma0=170,tdmae=6"
globals().update(knobs("TALL_KNOBS", {"ring": "RING", "b1": "B1_FIRST", "b1e": "B1_EVERY", "bar1": "BAR1_AFTER", "atail": "ATAIL",
                                      "adma0": "ADMA_FIRST", "admae": "ADMA_EVERY", "bdma0": "BDMA_FIRST", "bdmae": "BDMA_EVERY", "bar2": "BAR2_AFTER",
                                      "next": "NEXT_FIRST", "nexte": "NEXT_EVERY", "tdma0": "TDMA_FIRST", "tdmae": "TDMA_EVERY"}))
assert RING in (3, 4) and 0 <= ATAIL <= NA
read_slot = read_slot_from(S1)
LAYOUT = slot_layout(A_SLOTS, A_BYTES, B_BYTES, S1)


def acc(mi, ni):
    if mi < MI_AGPR:
        b = (mi * NI + ni) * 4
        return f"a[{b}:{b + 3}]"
    return vr(VACC + ((mi - MI_AGPR) * NI + ni) * 4)


def positions(first, every, n):
    return [first + k * every for k in range(n)]


def actions(m):
    """What follows MFMA m of a K-tile, in issue order. ("aread", dt, j): A fragment j = 12 ks + mi of tile t + dt into ring slot j % RING."""
    out = []
    if (m - 1) % NI == 0:
        j = (m - 1) // NI + RING - 1
        out.append(("aread", j // (2 * MI), j % (2 * MI)))
    if m in positions(B1_FIRST, B1_EVERY, NI):
        out.append(("bread", 0, 1, positions(B1_FIRST, B1_EVERY, NI).index(m)))
    if m == BAR1_AFTER:
        out.append(("bar1",))
    if m in positions(ADMA_FIRST, ADMA_EVERY, NA - ATAIL):
        out.append(("adma", 1, ATAIL + positions(ADMA_FIRST, ADMA_EVERY, NA - ATAIL).index(m)))
    if m in positions(BDMA_FIRST, BDMA_EVERY, NB):
        out.append(("bdma", 2, positions(BDMA_FIRST, BDMA_EVERY, NB).index(m)))
    if m == BAR2_AFTER:
        out.append(("bar2",))
    if m in positions(NEXT_FIRST, NEXT_EVERY, NI):
        out.append(("bread", 1, 0, positions(NEXT_FIRST, NEXT_EVERY, NI).index(m)))
    if m in positions(TDMA_FIRST, TDMA_EVERY, ATAIL):
        out.append(("adma", 2, positions(TDMA_FIRST, TDMA_EVERY, ATAIL).index(m)))
    return out


class Gen(Stream):
    A_SLOTS, A_BYTES, B_SLOTS, B_BYTES = A_SLOTS, A_BYTES, B_SLOTS, B_BYTES
    SOFF_A, SOFF_B, STAMP0 = SA, SB, STAMP0

    def addr(self, slot, kind, ks):
        if slot == 0:
            return f"%[{'fa' if kind == 'A' else 'fb'}{ks}]"
        return f"v{S1 + ks}" if kind == "A" else f"v{S1 + 2 + ks}"

    def read_a(self, t, j):
        ks, mi = divmod(j, MI)
        self.e(f"ds_read_b128 {vr(ARING + 4 * (j % RING))}, {self.addr(t % A_SLOTS, 'A', ks)} offset:{mi * 2048}")
        self.pending.append(("A", j))

    def read_b(self, t, ks, ni):
        self.e(f"ds_read_b128 {vr(BSET[ks] + 4 * ni)}, {self.addr(t % B_SLOTS, 'B', ks)} offset:{ni * 2048}")
        self.pending.append(("B", ks, ni))

    def body(self, p):
        """K-tile t with t % 2 == p."""
        e = self.e
        e(f"; ================= K-tile body {p}: A slot {1 - p} <- A(t+1), B slot {p} <- B(t+2), A slot {p} <- first pieces of A(t+2) =================")
        self.stamp(0, p)
        done = {"bar1": False, "bar2": False, "adma": 0, "bdma": 0, "tdma": 0, "bread1": 0, "bread0": 0}
        for m in range(1, NM + 1):
            j, ni = divmod(m - 1, NI)
            ks, mi = divmod(j, MI)
            if ni == 0:
                self.need(("A", j))
            if mi == 0:
                self.need(("B", ks, ni))
            e(f"v_mfma_f32_16x16x32_bf16 {acc(mi, ni)}, {vr(ARING + 4 * (j % RING))}, {vr(BSET[ks] + 4 * ni)}, {acc(mi, ni)}")
            for act in actions(m):
                if act[0] == "aread":
                    assert done["bar2"] == (act[1] == 1), "A fragments of tile t are read before the second barrier, those of tile t+1 behind it"
                    self.read_a(p + act[1], act[2])
                elif act[0] == "bread":
                    if act[1] == 0:   # k-step 1 of this tile: its registers are free once tile t-1 is multiplied, its slot until BAR1
                        assert not done["bar1"]
                        done["bread1"] += 1
                    else:             # k-step 0 of tile t+1: its registers are free behind MFMA 96, its slot is visible behind BAR2
                        assert done["bar2"] and m > MI * NI
                        done["bread0"] += 1
                    self.read_b(p + act[1], act[2], act[3])
                elif act[0] == "bar1":
                    assert done["bread1"] == NI
                    self.stamp(1, p)
                    self.wait_reads(max(i for i, n in enumerate(self.pending) if n[0] == "B"))   # both k-steps' B fragments are in registers
                    self.stamp(2, p)
                    e("s_barrier")                      # ... in every wave: B slot p may be overwritten
                    self.stamp(3, p)
                    done["bar1"] = True
                elif act[0] == "adma":
                    if act[1] == 1:   # the rest of A(t+1): behind BAR2 of tile t-1, before the first piece of B(t+2)
                        assert not done["bdma"] and not done["bar2"]
                        done["adma"] += 1
                    else:
                        assert done["bar2"]
                        done["tdma"] += 1
                    self.emit_all([self.dma_a(p + act[1], act[2])])
                elif act[0] == "bdma":
                    assert done["bar1"] and done["adma"] == NA - ATAIL and not done["bar2"]
                    done["bdma"] += 1
                    self.emit_all([self.dma_b(p + 2, act[2])])
                elif act[0] == "bar2":
                    assert done["bdma"] == NB and done["adma"] == NA - ATAIL
                    self.advance(SA, NA)
                    self.advance(SB, NB)
                    self.stamp(4, p)
                    e(f"s_waitcnt vmcnt({NB}) lgkmcnt(0)")   # A(t+1), B(t+1) have landed for this wave, B(t+2) may fly; its reads of A slot p are back
                    self.pending = []
                    self.stamp(5, p)
                    e("s_barrier")                      # ... and for every other wave
                    self.stamp(6, p)
                    done["bar2"] = True
        assert done["bar1"] and done["bar2"] and done["tdma"] == ATAIL and done["bread0"] == NI
        self.stamp(7, p)

    def build(self):
        e = self.e
        self.descriptors((("s36", "%[alo]"), ("s37", "%[ahi]"), ("s38", "%[arec]"), ("s39", "0x00020000"), ("s40", "%[blo]"),
                          ("s41", "%[bhi]"), ("s42", "%[brec]"), ("s43", "0x00020000"), ("s46", "%[nk]")))
        self.piece_offsets(SA, NA, "%[sa]")
        self.piece_offsets(SB, NB, "%[sb]")
        # issue order A0 B0 B1 + the first ATAIL pieces of A1: the same in-order history the loop's counted wait assumes
        self.emit_all(self.dma_a(0, i) for i in range(NA))
        self.advance(SA, NA)
        for t in (0, 1):
            self.emit_all(self.dma_b(t, i) for i in range(NB))
            self.advance(SB, NB)
        self.emit_all(self.dma_a(1, i) for i in range(ATAIL))
        for ks in range(2):
            e(f"v_add_u32 v{S1 + ks}, {A_BYTES}, %[fa{ks}]")
            e(f"v_add_u32 v{S1 + 2 + ks}, {B_BYTES}, %[fb{ks}]")
        for i in range(256):
            e(f"v_accvgpr_write_b32 a{i}, 0")
        for i in range((MI - MI_AGPR) * NI * 4):
            e(f"v_mov_b32 v{VACC + i}, 0")
        e(f"s_waitcnt vmcnt({NB + ATAIL})")     # A0 and B0 have landed (B1 and the first pieces of A1 may fly)
        e("s_barrier")
        # the reads a K-tile body issues for its successor behind BAR2, in the same order
        for m in range(BAR2_AFTER, NM + 1):
            for act in actions(m):
                if act[0] == "aread" and act[1] == 1:
                    self.read_a(0, act[2])
                elif act[0] == "bread" and act[1] == 1:
                    self.read_b(0, act[2], act[3])
        self.loop(2, 46, list(self.pending))
        e("s_waitcnt vmcnt(0) lgkmcnt(0)")   # nothing of this wave may land in LDS after the epilogue takes it over
        e("s_nop 7")                          # the last MFMAs' results are read by ds_write / v_accvgpr_read next
        e("s_nop 7")
        e("s_nop 7")
        e("s_barrier")                        # ... and nothing of any other wave: the accumulators below go into the K-tile slots
        for mi in range(MI_AGPR, MI):
            grp, half = divmod(mi - MI_AGPR, 2)
            for ni in range(NI):
                for r in range(4):   # the layout gemm_tall_384x256_dump.inc gives a 32-row group, 16 KB per group
                    e(f"ds_write_b32 %[sp], v{VACC + ((mi - MI_AGPR) * NI + ni) * 4 + r} offset:{grp * 16384 + ((half * 16 + r) * (16 * NI) + ni * 16) * 4}")
        e("s_waitcnt lgkmcnt(0)")
        self.store_stamps()
        return self.lines


def check_products(lines, iterations=3):
    """Every MFMA multiplies what it should: walks prologue + loop bodies tracking, per fragment register, which fragment the last
    ds_read put there (that it has returned is check_wait_coverage's register rule). An MFMA on accumulator (mi, ni) must find A
    fragment mi and B fragment ni of the SAME k-step and slot, and each accumulator must see (slot, k-step) = (0,0) (0,1) (1,0) (1,1)
    (0,0) ...: one chain per output element, K ascending."""
    seq = walk(lines, iterations)
    held, chain = {}, {}
    n_mfma = 0
    for pos, ins in enumerate(seq):
        mm = re.match(r"ds_read_b128 v\[(\d+):\d+\], (\S+) offset:(\d+)", ins)
        if mm:
            kind, slot, ks = read_slot(mm.group(2))
            held[int(mm.group(1))] = (kind, slot, ks, int(mm.group(3)) // 2048)
            continue
        mm = re.match(r"v_mfma_f32_16x16x32_bf16 ([av])\[(\d+):\d+\], v\[(\d+):\d+\], v\[(\d+):\d+\], ([av])\[(\d+):\d+\]", ins)
        if mm:
            n_mfma += 1
            f = int(mm.group(2)) // 4 if mm.group(1) == "a" else MI_AGPR * NI + (int(mm.group(2)) - VACC) // 4
            mi, ni = divmod(f, NI)
            ra, rb = int(mm.group(3)), int(mm.group(4))
            if (mm.group(1), mm.group(2)) != (mm.group(5), mm.group(6)) or not 0 <= mi < MI:
                raise WaitCoverageError(f"MFMA at {pos} does not accumulate in place: {ins}")
            a, b = held.get(ra), held.get(rb)
            if not a or not b or a[0] != "A" or b[0] != "B" or a[3] != mi or b[3] != ni or a[1:3] != b[1:3]:
                raise WaitCoverageError(f"MFMA at {pos} on accumulator ({mi}, {ni}) multiplies {a} by {b}")
            want = ((chain[f][0] + chain[f][1]) % 2, 1 - chain[f][1]) if f in chain else (0, 0)
            if a[1:3] != want:
                raise WaitCoverageError(f"MFMA at {pos}: accumulator ({mi}, {ni}) gets (slot, k-step) {a[1:3]}, expected {want}")
            chain[f] = a[1:3]
            continue
        if ins.startswith("v_mfma"):
            raise WaitCoverageError(f"MFMA at {pos} is not in the form the checker reads: {ins}")
    if n_mfma != iterations * 2 * NM or len(chain) != MI * NI:
        raise WaitCoverageError(f"checker saw {n_mfma} MFMAs on {len(chain)} accumulators - the stream format changed")
    return True


def dump_inc():
    """C++ side of the epilogue: if constexpr (grp == G): row fragments 2G, 2G+1 of a[0:255] -> the wave's LDS scratch (the 192 x 256
    kernel's dump, one 32-row group longer)."""
    out = ["// GENERATED by tools/gen_gemm_asm_tall.py - do not edit. if constexpr (grp == G): slabs 2G, 2G+1 of a[0:255] -> LDS scratch.\n"]
    for grp in range(MI_AGPR // 2):
        ins = []
        for half in range(2):
            mi = 2 * grp + half
            for ni in range(NI):
                base = (mi * NI + ni) * 4
                for r in range(4):
                    ins.append(f"v_accvgpr_read_b32 v{r}, a{base + r}")
                ins.append("s_nop 0")
                for r in range(4):
                    ins.append(f"ds_write_b32 %[sb], v{r} offset:{((half * 16 + r) * (16 * NI) + ni * 16) * 4}")
        ins.append("s_waitcnt lgkmcnt(0)")
        text = "".join(i + "\\n\\t" for i in ins)
        out.append(f'if constexpr (grp == {grp}) asm volatile("{text}" : : [sb] "v"(scr_lane) : "v0", "v1", "v2", "v3", "memory");\n')
    return "".join(out)


def main():
    # --inject-raw-race: the second barrier's wait leaves the activations of tile t+1 in flight
    lines = finish(Gen(STAMPS).build(), SAVE_M0, (f"s_waitcnt vmcnt({NB}) lgkmcnt(0)", f"s_waitcnt vmcnt({NB + 1}) lgkmcnt(0)"))
    stats = check_wait_coverage(lines, LAYOUT)
    check_products(lines)
    emit("gen_gemm_asm_tall.py", "main loop of gemm_bf16_kernel_tall (gemm.hip)", "gemm_tall_384x256", STAMPS or os.environ.get("TALL_KNOBS"), lines, stats,
         {"gemm_tall_384x256_clobbers.inc": clobbers_inc("gen_gemm_asm_tall.py", NV, 256, range(36, SAVE_M0 + 1)), "gemm_tall_384x256_dump.inc": dump_inc()})


if __name__ == "__main__":
    main()
