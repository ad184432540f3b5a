#!/usr/bin/env python3
"""Generates ltx-video-swift-mlx_amd/csrc/gemm_dtl_192x256.inc (+ _clobbers.inc): the gfx950 assembly main loop of
gemm_bf16_kernel_dtl (gemm_asm_tiles.inc, tile_cfg 75). The generated files are committed; the build does not run this script.

C[M][N] = A[M][K] . B[N][K]^T, bf16 in, f32 accumulate. Workgroup tile 192 x 256 (the DiT's 1536 rows x 8192 / 16384 columns are
exactly one / two rounds of 256 such tiles), four waves as 2 x 2 = ONE wave per SIMD, wave tile 96 x 128 = 6 x 8 accumulators of
v_mfma_f32_16x16x32_bf16 in 192 AGPRs, K-tiles of 64. Same LDS image as every other GEMM kernel of this library (128-byte rows,
16-byte chunks XOR-swizzled by (row >> 1) & 7 on the LDS-DMA source address, 8-row pieces of 1 KB per wave instruction), same
accumulator map as tools/gen_gemm_asm.py (a[(mi*8+ni)*4 ..]), so the epilogue of that kernel is reused.

Structure (what a 24 + 32 KB K-tile allows in 160 KB of LDS: TWO slots for the activations, THREE for the weights = 144 KB):
  * both k-steps' fragments of a K-tile live in REGISTERS (2 x (6 A + 8 B) x 4 VGPRs = 112): once a tile's 28 fragment reads have
    returned, its LDS slots are free, so the LDS-DMA of A tile t+2 and of B tile t+3 go into the slots tile t was multiplied from;
  * why three weight slots: in-kernel stamps + a K sweep of the first (two-slot) version showed a K-tile body of 1760 cycles when
    nothing is waited for (87 % MFMA duty) but 1.26-1.5 us per K-tile in the steady state: the loop runs at (bytes in flight per
    CU) / (latency of HBM-cold weights, ~1.9 us) - 84 KB in flight then, ~116 KB now. The weights are the cold operand (the
    activations are re-read by every column tile and come from L2 / the memory-side cache), so the third slot goes to them;
  * per K-tile t (A slot t % 2, B slot t % 3), 96 MFMAs per wave, in one in-order stream:
      MFMA  1..14   k-step 0 products, one ds_read of a k-step-1 fragment behind each
      after BAR1    s_waitcnt lgkmcnt(0) + s_barrier        every wave has tile t in registers: its slots are free   [WAR]
      then          6 LDS-DMA pieces of A(t+2), 8 of B(t+3), one behind every DMA_EVERY-th MFMA
      after BAR2    s_waitcnt vmcnt(22) + s_barrier         A(t+1) and B(t+1) have landed; B(t+2), A(t+2), B(t+3) may fly [RAW]
      MFMA 83..96   one ds_read of a k-step-0 fragment of tile t+1 behind each
    two barriers and no VALU instruction per K-tile; the loop body is six tiles long (2 x 3 slots), left after any tile. Every
    wait is derived from the issue order, and check_wait_coverage() (tools/asm_common.py, shared with every proven
    stream) proves both hazards and the operand waits on the emitted text before the file is written.

Register map (per wave):
  v[0:23]  A fragments k-step 0   v[24:55]  B fragments k-step 0      v[56:79] / v[80:111]  the same for k-step 1
  v[112:113] A slot 1, v[114:115] / v[116:117] B slots 1 / 2: copies of the fragment addresses     a[0:191] accumulators
  s[36:39] / s[40:43] A / B buffer descriptors   s46 tile counter   s[50:55] / s[56:63] scalar offsets of the A / B pieces
"""
import os
import sys

from asm_common import RegisterTileStream, check_wait_coverage, clobbers_inc, emit, finish, knobs, slot_layout

MI, NI = 6, 8
NA, NB = 6, 8                 # LDS-DMA pieces per wave and K-tile
A_BYTES = 192 * 128           # 24576 per A slot
B_BYTES = 256 * 128           # 32768 per B slot
A_SLOTS, B_SLOTS = 2, 3       # LDS: [A0][A1][B0][B1][B2] = 147456 bytes
SET = (0, 56)                 # register sets of the two k-steps: A at +0 (6 x 4), B at +24 (8 x 4)
S1 = 112                      # fragment addresses of the slots other than 0
NV = S1 + 6
INFLIGHT = NB + NA + NB       # B(t+2), A(t+2), B(t+3) may still fly when tile t+1 is read
SOFF = 50
SAVE_M0 = 82
READ_UNTIL = 14               # k-step-1 reads sit behind MFMAs 1..14
BAR1_AFTER = 22
DMA_FIRST, DMA_EVERY = 23, 3
BAR2_AFTER = 82
NEXT_FROM = 83
STAMPS = "--stamps" in sys.argv   # diagnostic build (tools/ubench/gemm_dtl_stamps.hip): s_memtime at the phase boundaries of body 0
# schedule knobs for A/B builds: DTL_KNOBS="bar1=26,dma0=28,dmae=4,bar2=82,next=83,reads=14"
globals().update(knobs("DTL_KNOBS", {"bar1": "BAR1_AFTER", "dma0": "DMA_FIRST", "dmae": "DMA_EVERY", "bar2": "BAR2_AFTER", "next": "NEXT_FROM",
                                     "reads": "READ_UNTIL"}))
LAYOUT = slot_layout(A_SLOTS, A_BYTES, B_BYTES, S1)


def acc(mi, ni):
    b = (mi * NI + ni) * 4
    return f"a[{b}:{b + 3}]"


class Gen(RegisterTileStream):
    A_SLOTS, A_BYTES, B_SLOTS, B_BYTES, MI, NI, NA, NB, SET, S1 = A_SLOTS, A_BYTES, B_SLOTS, B_BYTES, MI, NI, NA, NB, SET, S1
    SOFF_A, SOFF_B, STAMP0, B_AHEAD, INFLIGHT = SOFF, SOFF + NA, 64, 3, INFLIGHT
    READ_UNTIL, BAR1_AFTER, DMA_FIRST, DMA_EVERY, BAR2_AFTER, NEXT_FROM = READ_UNTIL, BAR1_AFTER, DMA_FIRST, DMA_EVERY, BAR2_AFTER, NEXT_FROM
    acc = staticmethod(acc)

    def build(self):
        e = self.e
        self.descriptors((("s36", "%[alo]"), ("s37", "%[ahi]"), ("s38", "%[arec]"), ("s39", "0x00020000"), ("s40", "%[blo]"),
                          ("s41", "%[bhi]"), ("s42", "%[brec]"), ("s43", "0x00020000"), ("s46", "%[nk]")))
        self.piece_offsets(SOFF, NA, "%[sa]")
        self.piece_offsets(SOFF + NA, NB, "%[sb]")
        # issue order A0 B0 A1 B1 B2: the same in-order history the loop's counted wait assumes
        for t, kinds in ((0, "AB"), (1, "AB"), (2, "B")):
            for kind in kinds:
                if kind == "A":
                    self.emit_all(self.dma_a(t, i) for i in range(NA))
                    self.advance(SOFF, NA)
                else:
                    self.emit_all(self.dma_b(t, i) for i in range(NB))
                    self.advance(SOFF + NA, NB)
        for ks in range(2):
            e(f"v_add_u32 v{S1 + ks}, {A_BYTES}, %[fa{ks}]")
            for slot in (1, 2):
                e(f"v_add_u32 v{S1 + 2 * slot + ks}, {slot * B_BYTES}, %[fb{ks}]")
        for i in range(MI * NI * 4):
            e(f"v_accvgpr_write_b32 a{i}, 0")
        e(f"s_waitcnt vmcnt({INFLIGHT})")     # A0 and B0 have landed (A1, B1, B2 = 6 + 8 + 8 pieces may fly)
        e("s_barrier")
        self.loop(A_SLOTS * B_SLOTS, 46, self.first_reads())
        e("s_waitcnt vmcnt(0) lgkmcnt(0)")   # nothing may land in LDS after the epilogue scratch takes it over
        e("s_nop 7")
        e("s_nop 7")
        self.store_stamps()
        return self.lines


def main():
    # --inject-raw-race: the second barrier's wait leaves A(t+1) in flight
    lines = finish(Gen(STAMPS).build(), SAVE_M0, (f"s_waitcnt vmcnt({INFLIGHT})", f"s_waitcnt vmcnt({INFLIGHT + NA})"))
    stats = check_wait_coverage(lines, LAYOUT)
    emit("gen_gemm_asm_dtl.py", "main loop of gemm_bf16_kernel_dtl (gemm.hip)", "gemm_dtl_192x256", STAMPS or os.environ.get("DTL_KNOBS"), lines, stats,
         {"gemm_dtl_192x256_clobbers.inc": clobbers_inc("gen_gemm_asm_dtl.py", NV, MI * NI * 4, range(36, SAVE_M0 + 1))})


if __name__ == "__main__":
    main()
