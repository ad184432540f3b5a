"""What tools/gen_gemm_asm_dtl.py (192 x 256), gen_gemm_asm_qkv.py (192 x 384) and gen_gemm_asm_tall.py (384 x 256) share: the pieces of
a stream every one of them emits, the static proof of its LDS-DMA / ds_read ordering, and the way a generated file is written or compared
with the committed one. The three scripts stay the entry points; each keeps its schedule, its register map and the proofs only it has.

The streams have one format. LDS holds A_SLOTS activation slots followed by B_SLOTS weight slots. A wave stages a K-tile with LDS-DMA
pieces (`s_add_u32 m0, %[wlds], <byte offset>` / `buffer_load_dwordx4 ... offen lds`) and reads fragments with
`ds_read_b128 v[..], <address> offset:<fragment * 2048>`, where the address operand of slot 0 is `%[fa<k-step>]` / `%[fb<k-step>]` and
those of the other slots are VGPR copies from v<S1> on. The loop lies between `10:` and `s_branch 10b` and is left through
`s_cbranch_scc1 20f` after any of its K-tile bodies.
"""
import collections
import os
import re
import sys

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "ltx-video-swift-mlx_amd", "csrc")


def vr(b, n=4):
    return f"v[{b}:{b + n - 1}]"


def knobs(env, names):
    """Schedule knobs of an A/B build, e.g. DTL_KNOBS="bar1=26,dma0=28": {global name: value} for the script's globals().update()."""
    out = {}
    for kv in filter(None, os.environ.get(env, "").split(",")):
        k, v = kv.split("=")
        if k not in names:
            raise SystemExit(f"unknown knob {k}")
        out[names[k]] = int(v)
    return out


class Stream:
    """The instruction list and what every generator emits into it. A subclass sets SOFF_A / SOFF_B (first scalar offset of the A / B
    pieces), STAMP0 (first SGPR of the s_memtime stamps) and the slot geometry A_SLOTS, A_BYTES, B_SLOTS, B_BYTES."""

    def __init__(self, stamps):
        self.lines = []
        self.pending = []   # names of LDS reads in issue order (they return in order)
        self.stamps = stamps

    def e(self, s):
        self.lines.append(s)

    def wait_reads(self, idx):
        """counted wait: pending[idx] (and every older read) has returned"""
        n = len(self.pending) - 1 - idx
        self.e(f"s_waitcnt lgkmcnt({min(n, 15)})")   # 4-bit field: a smaller count waits for more, never for less
        self.pending = self.pending[idx + 1:] if n <= 15 else self.pending[len(self.pending) - 15:]

    def need(self, name):
        """counted wait: the read of fragment `name` (and every older one) has returned"""
        if name in self.pending:
            self.wait_reads(len(self.pending) - 1 - self.pending[::-1].index(name))

    def dma(self, dst, voff, desc, soff):
        """one LDS-DMA piece: 8 rows of 128 bytes per wave -> LDS byte `dst` of the workgroup's image"""
        return [f"s_add_u32 m0, %[wlds], {dst}", "s_nop 0", f"buffer_load_dwordx4 %[{voff}], s[{desc}:{desc + 3}], s{soff} offen lds"]

    def dma_a(self, t, i):
        return self.dma((t % self.A_SLOTS) * self.A_BYTES + i * 4096, "ao", 36, self.SOFF_A + i)

    def dma_b(self, t, i):
        return self.dma(self.A_SLOTS * self.A_BYTES + (t % self.B_SLOTS) * self.B_BYTES + i * 4096, "bo", 40, self.SOFF_B + i)

    def emit_all(self, pieces):
        for piece in pieces:
            for ins in piece:
                self.e(ins)

    def descriptors(self, movs):
        for a, b in movs:
            self.e(f"s_mov_b32 {a}, {b}")

    def piece_offsets(self, first, n, step):
        """scalar offsets of n pieces 32 rows apart: s<first> = 0, s<first + i> = i * step"""
        self.e(f"s_mov_b32 s{first}, 0")
        for i in range(1, n):
            self.e(f"s_add_u32 s{first + i}, s{first + i - 1}, {step}")

    def advance(self, first, n):
        """the next K-tile: 128 bytes further in every row"""
        for i in range(n):
            self.e(f"s_add_u32 s{first + i}, s{first + i}, 128")

    def stamp(self, i, p):
        if self.stamps and p == 0:
            self.e(f"s_memtime s[{self.STAMP0 + 2 * i}:{self.STAMP0 + 1 + 2 * i}]")

    def loop(self, bodies, counter, entry):
        """10: body 0 .. body n-1, left after any of them when the tile counter reaches 0; every body starts from the reads `entry`"""
        self.e("10:")
        for p in range(bodies):
            self.pending = list(entry)
            self.body(p)
            assert self.pending == entry, "the loop body must leave the entry state it assumes"
            self.e(f"s_sub_u32 s{counter}, s{counter}, 1")
            self.e(f"s_cmp_eq_u32 s{counter}, 0")
            self.e("s_cbranch_scc1 20f")
        self.e("s_branch 10b")
        self.e("20:")

    def store_stamps(self):
        if self.stamps:   # lane 0 of every wave writes its 8 stamps of the last pass through body 0: dbg[8] u64
            for i in range(16):
                self.e(f"v_mov_b32 v{i}, s{self.STAMP0 + i}")
            self.e("v_mov_b32 v16, 0")
            for i in range(8):
                self.e(f"global_store_dwordx2 v16, v[{2 * i}:{2 * i + 1}], %[dbg] offset:{i * 8}")
            self.e("s_waitcnt vmcnt(0)")


class RegisterTileStream(Stream):
    """The K-tile body of the 192 x 256 and 192 x 384 streams: both k-steps' fragments of a K-tile live in registers (MI A and NI B
    fragments per k-step, register sets SET[k-step], A first), so a tile's slots are free once its reads have returned. Per K-tile t:
    the k-step-1 reads behind the first MFMAs; lgkmcnt(0) + barrier [WAR]; the LDS-DMA pieces of A(t+2) and B(t+B_AHEAD), one behind
    every DMA_EVERY-th MFMA; a counted vmcnt(INFLIGHT) + barrier [RAW]; the k-step-0 reads of tile t+1 behind the last MFMAs. Two
    barriers and no VALU instruction per K-tile. A subclass sets MI, NI, NA, NB, SET, S1, B_AHEAD, INFLIGHT, the schedule positions
    READ_UNTIL, BAR1_AFTER, DMA_FIRST, DMA_EVERY, BAR2_AFTER, NEXT_FROM and acc(mi, ni)."""

    def frag_reg(self, ks, kind, i):
        return self.SET[ks] + 4 * (i if kind == "A" else self.MI + i)

    def read_order(self):
        """fragment read order of one k-step: what the MFMA stream (ni outer, mi inner) needs first comes first"""
        return [("B", 0)] + [("A", i) for i in range(self.MI)] + [("B", i) for i in range(1, self.NI)]

    def addr(self, slot, kind, ks):
        if slot == 0:
            return f"%[{'fa' if kind == 'A' else 'fb'}{ks}]"
        return f"v{self.S1 + ks}" if kind == "A" else f"v{self.S1 + 2 * slot + ks}"

    def read(self, t, ks, kind, i):
        slot = t % (self.A_SLOTS if kind == "A" else self.B_SLOTS)
        self.e(f"ds_read_b128 {vr(self.frag_reg(ks, kind, i))}, {self.addr(slot, kind, ks)} offset:{i * 2048}")
        self.pending.append((ks, kind, i))

    def body(self, p):
        """K-tile t with t % (A_SLOTS * B_SLOTS) == p."""
        e = self.e
        e(f"; ================= K-tile body {p}: A slot {p % self.A_SLOTS} <- A(t+2), B slot {p % self.B_SLOTS} <- B(t+{self.B_AHEAD}) =================")
        m = 0
        self.stamp(0, p)
        k1 = self.read_order()      # k-step-1 fragments of this tile, still to read
        nxt = self.read_order()     # k-step-0 fragments of the next tile
        # A pieces first, then B: the counted wait at the second barrier may then leave the NEWER weight tile in flight
        dmas = [self.dma_a(p + 2, i) for i in range(self.NA)] + [self.dma_b(p + self.B_AHEAD, i) for i in range(self.NB)]
        for ks in range(2):
            for ni in range(self.NI):
                for mi in range(self.MI):
                    m += 1
                    if mi == 0:
                        self.need((ks, "B", ni))
                    if ni == 0:
                        self.need((ks, "A", mi))
                    e(f"v_mfma_f32_16x16x32_bf16 {self.acc(mi, ni)}, {vr(self.frag_reg(ks, 'A', mi))}, {vr(self.frag_reg(ks, 'B', ni))}, {self.acc(mi, ni)}")
                    if m <= self.READ_UNTIL and k1:
                        self.read(p, 1, *k1.pop(0))
                    if m == self.BAR1_AFTER:
                        assert not k1
                        self.stamp(1, p)
                        e("s_waitcnt lgkmcnt(0)")          # this wave holds all of tile t in registers
                        self.pending = []
                        self.stamp(2, p)
                        e("s_barrier")                      # ... and so does every other wave: the slots of tile t may be overwritten
                        self.stamp(3, p)
                    if m >= self.DMA_FIRST and (m - self.DMA_FIRST) % self.DMA_EVERY == 0 and dmas:
                        self.emit_all([dmas.pop(0)])
                    if m == self.BAR2_AFTER:
                        assert not dmas
                        self.advance(self.SOFF_A, self.NA)
                        self.advance(self.SOFF_B, self.NB)
                        self.stamp(4, p)
                        e(f"s_waitcnt vmcnt({self.INFLIGHT})")   # A(t+1), B(t+1) have landed for this wave; the newer pieces may fly
                        self.stamp(5, p)
                        e("s_barrier")                      # ... and for every other wave
                        self.stamp(6, p)
                    if m >= self.NEXT_FROM and nxt:
                        self.read(p + 1, 0, *nxt.pop(0))
        assert m == 2 * self.MI * self.NI and not nxt
        self.stamp(7, p)

    def first_reads(self):
        """the k-step-0 reads of tile 0: the entry state of the loop"""
        for kind, i in self.read_order():
            self.read(0, 0, kind, i)
        return list(self.pending)


# ---------------------------------------------------------------------------------------------------------------
# the proof
# ---------------------------------------------------------------------------------------------------------------
class WaitCoverageError(AssertionError):
    pass


Slots = collections.namedtuple("Slots", "a_slots a_bytes b_slots b_bytes read_slot")


def read_slot_from(s1):
    """address operand of a ds_read -> (kind, slot, k-step), for fragment addresses of slot 0 in %[fa0] %[fa1] %[fb0] %[fb1] and those of
    the other slots in v<s1>, v<s1 + 1> (A slot 1) and v<s1 + 2 slot>, v<s1 + 2 slot + 1> (B)"""
    def read_slot(a):
        if a.startswith("%[fa"):
            return "A", 0, int(a[4])
        if a.startswith("%[fb"):
            return "B", 0, int(a[4])
        r = int(a[1:]) - s1
        return ("A", 1, r) if r < 2 else ("B", r // 2, r % 2)
    return read_slot


def walk(lines, iterations, with_exit=True):
    """prologue + iterations x loop body (+ exit), branches not taken"""
    i10, ibr = lines.index("10:"), lines.index("s_branch 10b")
    return lines[:i10] + lines[i10 + 1:ibr] * iterations + (lines[ibr + 1:] if with_exit else [])


def retire(queue, ins, counter, state):
    """a counted s_waitcnt: all but the newest `count` operations of the in-order queue get `state`"""
    mm = re.search(counter + r"\((\d+)\)", ins)
    if not mm:
        return queue
    keep = int(mm.group(1))
    done, queue = (queue[:len(queue) - keep], queue[len(queue) - keep:]) if keep < len(queue) else ([], queue)
    for op in done:
        op["state"] = state
    return queue


def check_wait_coverage(lines, slots, iterations=3):
    """Static proof of the LDS-DMA / ds_read ordering of the emitted stream (same rules as tools/gen_attn_w48.py):
      RAW  a ds_read of slot s needs every LDS-DMA issued into s to be retired by a counted vmcnt wait that is followed by a barrier;
      WAR  an LDS-DMA into slot s needs every earlier ds_read of s to be retired by an lgkmcnt wait that is followed by a barrier;
           a ds_write (accumulators that leave through LDS) needs that of every slot, and every LDS-DMA to be visible.
    Walks prologue + iterations x loop body + exit with branches not taken."""
    seq = walk(lines, iterations)
    b_base = slots.a_slots * slots.a_bytes
    regions = [("A", i) for i in range(slots.a_slots)] + [("B", i) for i in range(slots.b_slots)]
    vm, lg, fills, reads = [], [], {r: [] for r in regions}, {r: [] for r in regions}
    m0 = None
    n_reads = n_dma = 0
    for pos, ins in enumerate(seq):
        mm = re.match(r"s_add_u32 m0, %\[wlds\], (\d+)", ins)
        if mm:
            m0 = int(mm.group(1))
            continue
        if ins.startswith("buffer_load_dwordx4") and ins.endswith("lds"):
            slot = ("A", m0 // slots.a_bytes) if m0 < b_base else ("B", (m0 - b_base) // slots.b_bytes)
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
            slot = slots.read_slot(mm.group(1))[:2]
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
        if ins.startswith("ds_write"):
            for s in regions:
                if any(f["state"] != "visible" for f in fills[s]) or any(r["state"] != "fenced" for r in reads[s]):
                    raise WaitCoverageError(f"WAR: ds_write at {pos} while slot {s} is still in use")
            continue
        if ins.startswith("s_waitcnt"):
            vm = retire(vm, ins, "vmcnt", "retired")
            lg = retire(lg, ins, "lgkmcnt", "done")
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
    the counted lgkmcnt waits; an MFMA that names a register whose read is still outstanding is an error. (A read that overwrites a
    register an earlier-issued MFMA still has to read cannot happen: MFMAs read their operands at issue, and the stream is in order.)"""
    out = []  # (first register) of outstanding reads, issue order
    n_mfma = 0
    for pos, ins in enumerate(walk(lines, 3, with_exit=False)):
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


# ---------------------------------------------------------------------------------------------------------------
# from a proven stream to the committed files
# ---------------------------------------------------------------------------------------------------------------
def finish(lines, save_m0, raw_race):
    """The asm block as the kernel includes it. m0 (the LDS-DMA destination) is a reserved register: naming it in the clobber list draws
    "-Winline-asm ... may lead to undefined behaviour" from the compiler, so the block saves it in an SGPR of its own and restores it on
    the way out; the surrounding HIP code sees m0 unchanged and the clobber list does not name it.
    Checker self-tests: --inject-raw-race replaces the loop's first `raw_race[0]` (the wait in front of the second barrier) by
    `raw_race[1]`, which leaves a part of tile t+1 in flight; --inject-war-race drops the loop's first barrier."""
    lines = [f"s_mov_b32 s{save_m0}, m0"] + lines + [f"s_mov_b32 m0, s{save_m0}"]
    if "--inject-raw-race" in sys.argv:
        lines[lines.index(raw_race[0], lines.index("10:"))] = raw_race[1]
    if "--inject-war-race" in sys.argv:
        del lines[lines.index("s_barrier", lines.index("10:"))]
    return lines


def clobbers_inc(script, nv, na, s_last):
    """v0 .. v<nv - 1>, a0 .. a<na - 1>, s36 .. s<s_last>, twelve per line"""
    clob = [f"v{i}" for i in range(nv)] + [f"a{i}" for i in range(na)] + [f"s{i}" for i in range(36, s_last + 1)] + ["vcc", "scc", "memory"]
    text = f"// GENERATED by tools/{script} - do not edit. Registers the assembly main loop assigns by hand.\n"
    for i in range(0, len(clob), 12):
        text += ", ".join('"' + c + '"' for c in clob[i:i + 12]) + ("," if i + 12 < len(clob) else "") + "\n"
    return text


def emit(script, kernel, stem, diag, lines, stats, others):
    """Writes csrc/<stem>.inc (the stream as string literals) and `others` ({file name: text}), or with --check compares them with the
    committed files. A diagnostic build (`diag`: --stamps or schedule knobs) goes to <stem>_stamps.inc, which is not committed, and
    writes nothing else."""
    text = f"// GENERATED by tools/{script} - do not edit. gfx950 assembly main loop of {kernel} (gemm.hip).\n"
    text += "".join('"' + ln + '\\n\\t"\n' for ln in lines)
    files = {stem + ("_stamps.inc" if diag else ".inc"): text}
    if "--check" in sys.argv or not diag:
        files.update(others)
    files = {os.path.join(CSRC, name): t for name, t in files.items()}
    if "--check" in sys.argv:
        same = all(os.path.exists(p) and open(p).read() == t for p, t in files.items())
        print(f"wait coverage ok: {stats}; committed output {'matches' if same else 'DIFFERS'}")
        sys.exit(0 if same else 4)
    for p, t in files.items():
        with open(p, "w") as f:
            f.write(t)
    if diag:
        print(f"{len(lines)} lines -> {os.path.normpath(next(iter(files)))}; {stats}")
    else:
        print(f"{len(lines)} lines, {sum(1 for ln in lines if 'v_mfma' in ln)} MFMAs; {stats}")
