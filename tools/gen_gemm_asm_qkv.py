#!/usr/bin/env python3
"""Generates ltx-video-swift-mlx_amd/csrc/gemm_qkv_192x384.inc (+ _clobbers.inc, _vread.inc): the gfx950 assembly main loop of
gemm_bf16_kernel_qkv (gemm.hip). The generated files are committed; the build does not run this script. Sibling of
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
    in flight. The loop body is two tiles long, left after either. check_wait_coverage() proves both hazards on the emitted text
    before the file is written.
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
import re
import sys

MI, NQ, NVF = 6, 8, 4
NI = NQ + NVF
NA, NB = 6, 12                # LDS-DMA pieces per wave and K-tile
A_BYTES = 192 * 128           # 24576 per A slot
B_BYTES = 384 * 128           # 49152 per B slot
A_SLOTS, B_SLOTS = 2, 2
B_BASE = A_SLOTS * A_BYTES    # LDS: [A0][A1][B0][B1] = 147456 bytes
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
for _kv in filter(None, os.environ.get("QKV_KNOBS", "").split(",")):
    _k, _v = _kv.split("=")
    _v = int(_v)
    if _k == "bar1": BAR1_AFTER = _v
    elif _k == "dma0": DMA_FIRST = _v
    elif _k == "dmae": DMA_EVERY = _v
    elif _k == "bar2": BAR2_AFTER = _v
    elif _k == "next": NEXT_FROM = _v
    elif _k == "reads": READ_UNTIL = _v


def vr(b, n=4):
    return f"v[{b}:{b + n - 1}]"


def acc(mi, ni):
    if ni < NQ:
        b = (mi * NQ + ni) * 4
        return f"a[{b}:{b + 3}]"
    vf = mi * NVF + (ni - NQ)
    if vf < 16:
        b = 192 + vf * 4
        return f"a[{b}:{b + 3}]"
    return vr(VACC + (vf - 16) * 4)


def frag_reg(ks, kind, i):
    return SET[ks] + (4 * i if kind == "A" else 24 + 4 * i)


# fragment read order of one k-step: what the MFMA stream (ni outer, mi inner) needs first comes first
READ_ORDER = [("B", 0)] + [("A", i) for i in range(MI)] + [("B", i) for i in range(1, NI)]


class Gen:
    def __init__(self):
        self.lines = []
        self.pending = []   # names of LDS reads in issue order (they return in order)

    def e(self, s):
        self.lines.append(s)

    def addr(self, slot, kind, ks):
        name = ("fa" if kind == "A" else "fb") + str(ks)
        if slot == 0:
            return f"%[{name}]"
        return f"v{S1 + ks}" if kind == "A" else f"v{S1 + 2 + ks}"

    def read(self, t, ks, kind, i):
        slot = t % (A_SLOTS if kind == "A" else B_SLOTS)
        self.e(f"ds_read_b128 {vr(frag_reg(ks, kind, i))}, {self.addr(slot, kind, ks)} offset:{i * 2048}")
        self.pending.append((ks, kind, i))

    def need(self, name):
        """counted wait: the read of fragment `name` (and every older one) has returned"""
        if name not in self.pending:
            return
        idx = len(self.pending) - 1 - self.pending[::-1].index(name)
        n = len(self.pending) - 1 - idx
        self.e(f"s_waitcnt lgkmcnt({min(n, 15)})")   # 4-bit field: a smaller count waits for more, never for less
        self.pending = self.pending[idx + 1:] if n <= 15 else self.pending[len(self.pending) - 15:]

    def dma_a(self, t, i):
        dst = (t % A_SLOTS) * A_BYTES + i * 4096
        return [f"s_add_u32 m0, %[wlds], {dst}", "s_nop 0", f"buffer_load_dwordx4 %[ao], s[36:39], s{SA + i} offen lds"]

    def dma_b(self, t, i):
        dst = B_BASE + (t % B_SLOTS) * B_BYTES + i * 4096
        src, j = B_PIECE[i]
        if src == "q":
            return [f"s_add_u32 m0, %[wlds], {dst}", "s_nop 0", f"buffer_load_dwordx4 %[bo], s[40:43], s{SQ + j} offen lds"]
        return [f"s_add_u32 m0, %[wlds], {dst}", "s_nop 0", f"buffer_load_dwordx4 %[vo], s[44:47], s{SV + j} offen lds"]

    def advance_a(self):
        for i in range(NA):
            self.e(f"s_add_u32 s{SA + i}, s{SA + i}, 128")

    def advance_b(self):
        for i in range(NQ + NVF):
            self.e(f"s_add_u32 s{SQ + i}, s{SQ + i}, 128")   # the q|k and V offsets are neighbours: s56..s67

    def stamp(self, i, p):
        if STAMPS and p == 0:
            self.e(f"s_memtime s[{STAMP0 + 2 * i}:{STAMP0 + 1 + 2 * i}]")

    def body(self, p):
        """K-tile t with t % 2 == p."""
        e = self.e
        e(f"; ================= K-tile body {p}: A slot {p % A_SLOTS} <- A(t+2), B slot {p % B_SLOTS} <- B(t+2) =================")
        m = 0
        self.stamp(0, p)
        k1 = list(READ_ORDER)       # k-step-1 fragments of this tile, still to read
        nxt = list(READ_ORDER)      # k-step-0 fragments of the next tile
        dmas = [self.dma_a(p + 2, i) for i in range(NA)] + [self.dma_b(p + 2, i) for i in range(NB)]
        for ks in range(2):
            for ni in range(NI):
                for mi in range(MI):
                    m += 1
                    if mi == 0:
                        self.need((ks, "B", ni))
                    if ni == 0:
                        self.need((ks, "A", mi))
                    e(f"v_mfma_f32_16x16x32_bf16 {acc(mi, ni)}, {vr(frag_reg(ks, 'A', mi))}, {vr(frag_reg(ks, 'B', ni))}, {acc(mi, ni)}")
                    if m <= READ_UNTIL and k1:
                        kind, i = k1.pop(0)
                        self.read(p, 1, kind, i)
                    if m == BAR1_AFTER:
                        assert not k1
                        self.stamp(1, p)
                        e("s_waitcnt lgkmcnt(0)")          # this wave holds all of tile t in registers
                        self.pending = []
                        self.stamp(2, p)
                        e("s_barrier")                      # ... and so does every other wave: both slots p may be overwritten
                        self.stamp(3, p)
                    if m >= DMA_FIRST and (m - DMA_FIRST) % DMA_EVERY == 0 and dmas:
                        for ins in dmas.pop(0):
                            e(ins)
                    if m == BAR2_AFTER:
                        assert not dmas
                        self.advance_a()
                        self.advance_b()
                        self.stamp(4, p)
                        e(f"s_waitcnt vmcnt({INFLIGHT})")   # A(t+1), B(t+1) have landed for this wave; A(t+2), B(t+2) may fly
                        self.stamp(5, p)
                        e("s_barrier")                      # ... and for every other wave
                        self.stamp(6, p)
                    if m >= NEXT_FROM and nxt:
                        kind, i = nxt.pop(0)
                        self.read(p + 1, 0, kind, i)
        assert m == 2 * MI * NI and not nxt
        self.stamp(7, p)

    def build(self):
        e = self.e
        for a, b in (("s36", "%[alo]"), ("s37", "%[ahi]"), ("s38", "%[arec]"), ("s39", "0x00020000"), ("s40", "%[blo]"),
                     ("s41", "%[bhi]"), ("s42", "%[brec]"), ("s43", "0x00020000"), ("s44", "%[vlo]"), ("s45", "%[vhi]"),
                     ("s46", "%[vrec]"), ("s47", "0x00020000"), ("s48", "%[nk]")):
            e(f"s_mov_b32 {a}, {b}")
        for first, n, step in ((SA, NA, "%[sa]"), (SQ, NQ, "%[sb]"), (SV, NVF, "%[sv]")):
            e(f"s_mov_b32 s{first}, 0")
            for i in range(1, n):
                e(f"s_add_u32 s{first + i}, s{first + i - 1}, {step}")
        # issue order A0 B0 A1 B1: the same in-order history the loop's counted wait assumes
        for t in (0, 1):
            for kind in "AB":
                for i in range(NA if kind == "A" else NB):
                    for ins in (self.dma_a(t, i) if kind == "A" else self.dma_b(t, i)):
                        e(ins)
                self.advance_a() if kind == "A" else self.advance_b()
        for ks in range(2):
            e(f"v_add_u32 v{S1 + ks}, {A_BYTES}, %[fa{ks}]")
            e(f"v_add_u32 v{S1 + 2 + ks}, {B_BYTES}, %[fb{ks}]")
        for i in range(256):
            e(f"v_accvgpr_write_b32 a{i}, 0")
        for i in range(32):
            e(f"v_mov_b32 v{VACC + i}, 0")
        e(f"s_waitcnt vmcnt({INFLIGHT})")     # A0 and B0 have landed (A1, B1 = 6 + 12 pieces may fly)
        e("s_barrier")
        for kind, i in READ_ORDER:
            self.read(0, 0, kind, i)
        entry = list(self.pending)
        e("10:")
        for p in range(2):
            self.pending = list(entry)
            self.body(p)
            assert self.pending == entry, "the loop body must leave the entry state it assumes"
            e("s_sub_u32 s48, s48, 1")
            e("s_cmp_eq_u32 s48, 0")
            e("s_cbranch_scc1 20f")
        e("s_branch 10b")
        e("20:")
        e("s_waitcnt vmcnt(0) lgkmcnt(0)")   # nothing of this wave may land in LDS after the epilogue takes it over
        e("s_nop 7")                          # the last MFMAs' results are read by ds_write / v_accvgpr_read next
        e("s_nop 7")
        e("s_nop 7")
        e("s_barrier")                        # ... and nothing of any other wave: the spill below lies inside the K-tile slots
        for j in range(8):
            e(f"ds_write_b128 %[sp], {vr(VACC + 4 * j)} offset:{j * 1024}")
        e("s_waitcnt lgkmcnt(0)")
        if STAMPS:   # lane 0 of every wave writes its 8 stamps of the last pass through body 0: dbg[8] u64
            for i in range(16):
                e(f"v_mov_b32 v{i}, s{STAMP0 + i}")
            e("v_mov_b32 v16, 0")
            for i in range(8):
                e(f"global_store_dwordx2 v16, v[{2 * i}:{2 * i + 1}], %[dbg] offset:{i * 8}")
            e("s_waitcnt vmcnt(0)")
        return self.lines


class WaitCoverageError(AssertionError):
    pass


def check_wait_coverage(lines, iterations=3):
    """Static proof of the LDS-DMA / ds_read ordering of the emitted stream (same rules as tools/gen_gemm_asm_dtl.py):
      RAW  a ds_read of slot s needs every LDS-DMA issued into s to be retired by a counted vmcnt wait that is followed by a barrier;
      WAR  an LDS-DMA into slot s needs every earlier ds_read of s to be retired by an lgkmcnt wait that is followed by a barrier.
    Walks prologue + iterations x loop body + exit with branches not taken."""
    i10, ibr = lines.index("10:"), lines.index("s_branch 10b")
    seq = lines[:i10] + lines[i10 + 1:ibr] * iterations + lines[ibr + 1:]
    regions = [("A", i) for i in range(A_SLOTS)] + [("B", i) for i in range(B_SLOTS)]
    vm, lg, fills, reads = [], [], {r: [] for r in regions}, {r: [] for r in regions}
    m0 = None
    n_reads = n_dma = 0
    for pos, ins in enumerate(seq):
        mm = re.match(r"s_add_u32 m0, %\[wlds\], (\d+)", ins)
        if mm:
            m0 = int(mm.group(1))
            continue
        if ins.startswith("buffer_load_dwordx4") and ins.endswith("lds"):
            slot = ("A", m0 // A_BYTES) if m0 < B_BASE else ("B", (m0 - B_BASE) // B_BYTES)
            for r in reads[slot]:
                if r["state"] != "fenced":
                    raise WaitCoverageError(f"WAR: LDS-DMA into slot {slot} at {pos} while the ds_read at {r['pos']} is only '{r['state']}'")
            reads[slot] = []
            op = {"state": "inflight", "pos": pos}
            vm.append(op)
            fills[slot].append(op)
            n_dma += 1
            m0 = None
            continue
        mm = re.match(r"ds_read_b128 v\[\d+:\d+\], (\S+) offset:(\d+)", ins)
        if mm:
            a = mm.group(1)
            if a.startswith("%[fa"):
                slot = ("A", 0)
            elif a.startswith("%[fb"):
                slot = ("B", 0)
            else:
                slot = ("A", 1) if int(a[1:]) - S1 < 2 else ("B", 1)
            if not fills[slot]:
                raise WaitCoverageError(f"RAW: ds_read of slot {slot} at {pos} before anything was staged")
            for f in fills[slot]:
                if f["state"] != "visible":
                    raise WaitCoverageError(f"RAW: ds_read of slot {slot} at {pos} ({ins}) while the LDS-DMA at {f['pos']} is only '{f['state']}'")
            op = {"state": "issued", "pos": pos}
            lg.append(op)
            reads[slot].append(op)
            n_reads += 1
            continue
        if ins.startswith("s_waitcnt"):
            mv, ml = re.search(r"vmcnt\((\d+)\)", ins), re.search(r"lgkmcnt\((\d+)\)", ins)
            if mv:
                keep = int(mv.group(1))
                done, vm = (vm[:len(vm) - keep], vm[len(vm) - keep:]) if keep < len(vm) else ([], vm)
                for op in done:
                    op["state"] = "retired"
            if ml:
                keep = int(ml.group(1))
                done, lg = (lg[:len(lg) - keep], lg[len(lg) - keep:]) if keep < len(lg) else ([], lg)
                for op in done:
                    op["state"] = "done"
            continue
        if ins == "s_barrier":
            for s in regions:
                for op in fills[s]:
                    if op["state"] == "retired":
                        op["state"] = "visible"
                for op in reads[s]:
                    if op["state"] == "done":
                        op["state"] = "fenced"
    if not n_reads or not n_dma:
        raise WaitCoverageError("checker saw no LDS traffic - the stream format changed")
    return {"reads": n_reads, "fills": n_dma, "instructions": len(seq)}


def check_operand_waits(lines):
    """Every MFMA operand fragment must have returned from LDS: walk one prologue + 3 loop bodies, tracking reads in issue order and
    the counted lgkmcnt waits; an MFMA that names a register whose read is still outstanding is an error."""
    i10, ibr = lines.index("10:"), lines.index("s_branch 10b")
    seq = lines[:i10] + lines[i10 + 1:ibr] * 3
    out = []  # (first register) of outstanding reads, issue order
    n_mfma = 0
    for pos, ins in enumerate(seq):
        mm = re.match(r"ds_read_b128 v\[(\d+):\d+\]", ins)
        if mm:
            out.append(int(mm.group(1)))
            continue
        ml = re.search(r"lgkmcnt\((\d+)\)", ins) if ins.startswith("s_waitcnt") else None
        if ml:
            keep = int(ml.group(1))
            out = out[len(out) - keep:] if keep < len(out) else out
            continue
        mm = re.match(r"v_mfma_f32_16x16x32_bf16 [av]\[\d+:\d+\], v\[(\d+):\d+\], v\[(\d+):\d+\]", ins)
        if mm:
            n_mfma += 1
            for r in (int(mm.group(1)), int(mm.group(2))):
                if r in out:
                    raise WaitCoverageError(f"MFMA at {pos} reads v[{r}:{r + 3}] while its ds_read is outstanding")
            continue
        if ins.startswith("v_mfma"):
            raise WaitCoverageError(f"MFMA at {pos} is not in the form the checker reads: {ins}")
    if not n_mfma:
        raise WaitCoverageError("checker saw no MFMA - the stream format changed")
    return True


def vread_inc():
    """C++ side of the V epilogue: fragment vf (row slab vf / 4, column fragment vf % 4) of a[192:255] -> floats f0..f3."""
    out = ["// GENERATED by tools/gen_gemm_asm_qkv.py - do not edit. if constexpr (vf == F): V accumulator F of a[192:255] -> f0..f3.\n"]
    for vf in range(16):
        b = 192 + vf * 4
        reads = "".join(f"v_accvgpr_read_b32 %{r}, a{b + r}\\n\\t" for r in range(4))
        out.append(f'if constexpr (vf == {vf}) asm volatile("{reads}" : "=v"(f0), "=v"(f1), "=v"(f2), "=v"(f3));\n')
    return "".join(out)


def main():
    g = Gen()
    lines = g.build()
    # m0 (the LDS-DMA destination) is a reserved register: the block saves it in an SGPR of its own and restores it on the way out,
    # so the surrounding HIP code sees m0 unchanged and the clobber list does not name it
    lines = [f"s_mov_b32 s{SAVE_M0}, m0"] + lines + [f"s_mov_b32 m0, s{SAVE_M0}"]
    if "--inject-raw-race" in sys.argv:   # checker self-test: the second barrier's wait leaves the weights of tile t+1 in flight
        k = lines.index(f"s_waitcnt vmcnt({INFLIGHT})", lines.index("10:"))
        lines[k] = f"s_waitcnt vmcnt({INFLIGHT + NB})"
    if "--inject-war-race" in sys.argv:   # checker self-test: the first barrier is dropped
        k = lines.index("s_barrier", lines.index("10:"))
        del lines[k]
    stats = check_wait_coverage(lines)
    check_operand_waits(lines)
    here = os.path.dirname(os.path.abspath(__file__))
    d = os.path.join(here, "..", "ltx-video-swift-mlx_amd", "csrc")
    body = ["// GENERATED by tools/gen_gemm_asm_qkv.py - do not edit. gfx950 assembly main loop of gemm_bf16_kernel_qkv (gemm.hip).\n"]
    body += ['"' + ln + '\\n\\t"\n' for ln in lines]
    diag = STAMPS or os.environ.get("QKV_KNOBS")
    path = os.path.join(d, "gemm_qkv_192x384_stamps.inc" if diag else "gemm_qkv_192x384.inc")
    clob = [f"v{i}" for i in range(NV)] + [f"a{i}" for i in range(256)] + [f"s{i}" for i in range(36, SAVE_M0 + 1)] + ["vcc", "scc", "memory"]
    clob_text = "// GENERATED by tools/gen_gemm_asm_qkv.py - do not edit. Registers the assembly main loop assigns by hand.\n"
    for i in range(0, len(clob), 12):
        clob_text += ", ".join('"' + c + '"' for c in clob[i:i + 12]) + ("," if i + 12 < len(clob) else "") + "\n"
    if "--check" in sys.argv:
        others = ((os.path.join(d, "gemm_qkv_192x384_clobbers.inc"), clob_text), (os.path.join(d, "gemm_qkv_192x384_vread.inc"), vread_inc()))
        same = os.path.exists(path) and open(path).read() == "".join(body)
        same = same and all(os.path.exists(p) and open(p).read() == t for p, t in others)
        print(f"wait coverage ok: {stats}; committed files {'match' if same else 'DIFFER'}")
        sys.exit(0 if same else 4)
    with open(path, "w") as f:
        f.write("".join(body))
    if diag:
        print(f"{len(lines)} lines -> {os.path.normpath(path)}; {stats}")
        return
    with open(os.path.join(d, "gemm_qkv_192x384_clobbers.inc"), "w") as f:
        f.write(clob_text)
    with open(os.path.join(d, "gemm_qkv_192x384_vread.inc"), "w") as f:
        f.write(vread_inc())
    print(f"{len(lines)} lines, {sum(1 for ln in lines if 'v_mfma' in ln)} MFMAs; {stats}")


if __name__ == "__main__":
    main()
