#!/usr/bin/env python3
"""Generates ltx-video-swift-mlx_amd/csrc/gemm_qkv_192x384.inc (+ _clobbers.inc, _vread.inc): the gfx950 assembly main loop of
gemm_bf16_kernel_qkv (gemm_asm_tiles.inc). The generated files are committed; the build does not run this script. Sibling of
tools/gen_gemm_asm_dtl.py (the 192 x 256 stream), whose output this script never touches.

One launch for the self-attention projections q|k (N = 2 D, row-major bf16 store) and V (N = D, transposed bf16 store) of a DiT block:
both read the same adaLN rows. Workgroup tile 192 rows x 384 columns = 256 columns of the fused q|k matrix + 128 columns of V, taken
through TWO weight descriptors (the resident weights stay as they are); 1536 rows x (8192 + 4096) columns are exactly one round of
256 such tiles. Four waves as 2 x 2 = ONE wave per SIMD, wave tile 96 x 192 = 6 x 12 accumulators of v_mfma_f32_16x16x32_bf16,
K-tiles of 64, the LDS image of every other GEMM kernel of this library (128-byte rows, 16-byte chunks XOR-swizzled by (row >> 1) & 7
on the LDS-DMA source address, 8-row pieces of 1 KB per wave instruction).

The 384 weight rows of a K-tile lie in LDS as [q|k 0..127][V 0..63][q|k 128..255][V 64..127]: the column range of wave column wc is
LDS rows [192 wc, 192 wc + 192) = fragments 0..7 of q|k and 8..11 of V, so which epilogue a fragment gets is a compile-time fact.
LDS-DMA piece i of wave w is LDS rows (w + 4 i) * 8 .. + 7, hence pieces 0-3 and 6-9 come from q|k (scalar offsets of 32-row steps,
as in the 192 x 256 stream) and pieces 4-5 and 10-11 from V.

Structure (a 24 + 48 KB K-tile in 160 KB of LDS: TWO slots for the activations and TWO for the weights = 144 KB; a third weight slot
does not fit):
  * both k-steps' fragments of a K-tile live in REGISTERS (2 x (6 A + 12 B) x 4 VGPRs = 144): once a tile's 36 fragment reads have
    returned its LDS slots are free, and the LDS-DMA of A(t+2) and B(t+2) goes into the slots tile t was multiplied from;
  * per K-tile t (A and B slot t % 2), 144 MFMAs per wave, 18 fragment reads per 72 MFMAs, in one in-order stream:
      MFMA   1..18   k-step 0 products, one ds_read of a k-step-1 fragment behind each
      after BAR1     s_waitcnt lgkmcnt(0) + s_barrier        every wave has tile t in registers: its slots are free   [WAR]
      then           6 LDS-DMA pieces of A(t+2), 12 of B(t+2), one behind every DMA_EVERY-th MFMA
      after BAR2     s_waitcnt vmcnt(18) + s_barrier         A(t+1) and B(t+1) have landed; A(t+2), B(t+2) may fly    [RAW]
      MFMA 127..144  one ds_read of a k-step-0 fragment of tile t+1 behind each
    B(t+2) can only be requested after the barrier that frees tile t, so the counted wait leaves exactly the 18 pieces of tile t+2
    in flight. The loop body is two tiles long, left after either. check_wait_coverage() (tools/asm_common.py, shared with
    every proven stream) proves both hazards and the operand waits on the emitted text before the file is written.
  * one accumulator chain per output element, K ascending, A = activations, B = weights: bit-identical to the 192 x 256 stream
    and to the 192 x 128 ring kernel on the same operands.

Register map (per wave):
  v[0:23] A / v[24:71] B fragments of k-step 0    v[72:95] / v[96:143] the same for k-step 1
  a[0:191]    q|k accumulators, a[(mi*8 + ni)*4 ..]: the map of the 192 x 256 stream (its LDS dump is reused by the epilogue)
  a[192:255]  V accumulators of row slabs 0..3, a[192 + (mi*4 + nv)*4 ..]
  v[144:175]  V accumulators of row slabs 4, 5 (288 accumulator registers do not fit 256 AGPRs). The C++ epilogue behind the asm
              block cannot see clobbered VGPRs, so the stream ends by writing these eight fragments to LDS ([sp] + 1 KB each, behind
              a barrier: every wave's LDS-DMA has landed, no slot is read any more), where the epilogue reads them back.
  v[176:177] / v[178:179] fragment addresses of A / B slot 1
  s[36:39] / s[40:43] / s[44:47] A / q|k / V buffer descriptors   s48 tile counter
  s[50:55] / s[56:63] / s[64:67] scalar offsets of the A / q|k / V pieces
"""
import os
import sys

from asm_common import RegisterTileStream, check_wait_coverage, clobbers_inc, emit, finish, knobs, slot_layout, vr

MI, NQ, NVF = 6, 8, 4
NI = NQ + NVF
NA, NB = 6, 12                # LDS-DMA pieces per wave and K-tile
A_BYTES = 192 * 128           # 24576 per A slot
B_BYTES = 384 * 128           # 49152 per B slot
A_SLOTS, B_SLOTS = 2, 2       # LDS: [A0][A1][B0][B1] = 147456 bytes
SET = (0, 72)                 # register sets of the two k-steps: A at +0 (6 x 4), B at +24 (12 x 4)
VACC = 144                    # the eight V accumulators that do not fit the AGPRs
S1 = 176                      # fragment addresses of slot 1
NV = S1 + 4
INFLIGHT = NA + NB            # A(t+2), B(t+2) may still fly when tile t+1 is read
SA, SQ, SV = 50, 56, 64       # first scalar offset of the A / q|k / V pieces
STAMP0, SAVE_M0 = 68, 84
# piece i of the 12 B pieces -> (source, index of its scalar offset)
B_PIECE = [("q", i) for i in range(4)] + [("v", 0), ("v", 1)] + [("q", i) for i in range(4, 8)] + [("v", 2), ("v", 3)]
READ_UNTIL = 18               # k-step-1 reads sit behind MFMAs 1..18
BAR1_AFTER = 26
DMA_FIRST, DMA_EVERY = 27, 5
BAR2_AFTER = 126
NEXT_FROM = 127
STAMPS = "--stamps" in sys.argv   # diagnostic build (tools/ubench/gemm_qkv_stamps.hip): s_memtime at the phase boundaries of body 0
# schedule knobs for A/B builds: QKV_KNOBS="bar1=26,dma0=27,dmae=5,bar2=126,next=127,reads=18"
globals().update(knobs("QKV_KNOBS", {"bar1": "BAR1_AFTER", "dma0": "DMA_FIRST", "dmae": "DMA_EVERY", "bar2": "BAR2_AFTER", "next": "NEXT_FROM",
                                     "reads": "READ_UNTIL"}))
LAYOUT = slot_layout(A_SLOTS, A_BYTES, B_BYTES, S1)


def acc(mi, ni):
    if ni < NQ:
        b = (mi * NQ + ni) * 4
        return f"a[{b}:{b + 3}]"
    vf = mi * NVF + (ni - NQ)
    if vf < 16:
        b = 192 + vf * 4
        return f"a[{b}:{b + 3}]"
    return vr(VACC + (vf - 16) * 4)


class Gen(RegisterTileStream):
    A_SLOTS, A_BYTES, B_SLOTS, B_BYTES, MI, NI, NA, NB, SET, S1 = A_SLOTS, A_BYTES, B_SLOTS, B_BYTES, MI, NI, NA, NB, SET, S1
    SOFF_A, SOFF_B, STAMP0, B_AHEAD, INFLIGHT = SA, SQ, STAMP0, 2, INFLIGHT   # the q|k and V offsets are neighbours: s56..s67
    READ_UNTIL, BAR1_AFTER, DMA_FIRST, DMA_EVERY, BAR2_AFTER, NEXT_FROM = READ_UNTIL, BAR1_AFTER, DMA_FIRST, DMA_EVERY, BAR2_AFTER, NEXT_FROM
    acc = staticmethod(acc)

    def dma_b(self, t, i):
        dst = A_SLOTS * A_BYTES + (t % B_SLOTS) * B_BYTES + i * 4096
        src, j = B_PIECE[i]
        return self.dma(dst, "bo", 40, SQ + j) if src == "q" else self.dma(dst, "vo", 44, SV + j)

    def build(self):
        e = self.e
        self.descriptors((("s36", "%[alo]"), ("s37", "%[ahi]"), ("s38", "%[arec]"), ("s39", "0x00020000"), ("s40", "%[blo]"),
                          ("s41", "%[bhi]"), ("s42", "%[brec]"), ("s43", "0x00020000"), ("s44", "%[vlo]"), ("s45", "%[vhi]"),
                          ("s46", "%[vrec]"), ("s47", "0x00020000"), ("s48", "%[nk]")))
        for first, n, step in ((SA, NA, "%[sa]"), (SQ, NQ, "%[sb]"), (SV, NVF, "%[sv]")):
            self.piece_offsets(first, n, step)
        # issue order A0 B0 A1 B1: the same in-order history the loop's counted wait assumes
        for t in (0, 1):
            self.emit_all(self.dma_a(t, i) for i in range(NA))
            self.advance(SA, NA)
            self.emit_all(self.dma_b(t, i) for i in range(NB))
            self.advance(SQ, NB)
        for ks in range(2):
            e(f"v_add_u32 v{S1 + ks}, {A_BYTES}, %[fa{ks}]")
            e(f"v_add_u32 v{S1 + 2 + ks}, {B_BYTES}, %[fb{ks}]")
        for i in range(256):
            e(f"v_accvgpr_write_b32 a{i}, 0")
        for i in range(32):
            e(f"v_mov_b32 v{VACC + i}, 0")
        e(f"s_waitcnt vmcnt({INFLIGHT})")     # A0 and B0 have landed (A1, B1 = 6 + 12 pieces may fly)
        e("s_barrier")
        self.loop(2, 48, self.first_reads())
        e("s_waitcnt vmcnt(0) lgkmcnt(0)")   # nothing of this wave may land in LDS after the epilogue takes it over
        e("s_nop 7")                          # the last MFMAs' results are read by ds_write / v_accvgpr_read next
        e("s_nop 7")
        e("s_nop 7")
        e("s_barrier")                        # ... and nothing of any other wave: the spill below lies inside the K-tile slots
        for j in range(8):
            e(f"ds_write_b128 %[sp], {vr(VACC + 4 * j)} offset:{j * 1024}")
        e("s_waitcnt lgkmcnt(0)")
        self.store_stamps()
        return self.lines


def vread_inc():
    """C++ side of the V epilogue: fragment vf (row slab vf / 4, column fragment vf % 4) of a[192:255] -> floats f0..f3."""
    out = ["// GENERATED by tools/gen_gemm_asm_qkv.py - do not edit. if constexpr (vf == F): V accumulator F of a[192:255] -> f0..f3.\n"]
    for vf in range(16):
        b = 192 + vf * 4
        reads = "".join(f"v_accvgpr_read_b32 %{r}, a{b + r}\\n\\t" for r in range(4))
        out.append(f'if constexpr (vf == {vf}) asm volatile("{reads}" : "=v"(f0), "=v"(f1), "=v"(f2), "=v"(f3));\n')
    return "".join(out)


def main():
    # --inject-raw-race: the second barrier's wait leaves the weights of tile t+1 in flight
    lines = finish(Gen(STAMPS).build(), SAVE_M0, (f"s_waitcnt vmcnt({INFLIGHT})", f"s_waitcnt vmcnt({INFLIGHT + NB})"))
    stats = check_wait_coverage(lines, LAYOUT)
    emit("gen_gemm_asm_qkv.py", "main loop of gemm_bf16_kernel_qkv (gemm.hip)", "gemm_qkv_192x384", STAMPS or os.environ.get("QKV_KNOBS"), lines, stats,
         {"gemm_qkv_192x384_clobbers.inc": clobbers_inc("gen_gemm_asm_qkv.py", NV, 256, range(36, SAVE_M0 + 1)), "gemm_qkv_192x384_vread.inc": vread_inc()})


if __name__ == "__main__":
    main()
