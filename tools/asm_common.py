"""What the five generators of proven gfx950 assembly share - tools/gen_attn_w48.py and gen_attn_x32.py (attention), gen_gemm_asm_dtl.py
(192 x 256), gen_gemm_asm_qkv.py (192 x 384) and gen_gemm_asm_tall.py (384 x 256): the static proof of a stream's LDS ordering and
register use, for which a generator only declares its LDS layout; the way a generated file is written or compared with the committed
one; and the pieces of a stream the three GEMM generators emit. The scripts stay the entry points; each keeps its schedule, its register
map and the proofs only it has.

The GEMM streams have one format. LDS holds A_SLOTS activation slots followed by B_SLOTS weight slots. A wave stages a K-tile with LDS-DMA
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


# What a generator declares about its LDS: fill(byte offset in m0 of an LDS-DMA) -> region; read(address operand, offset of an LDS
# read) -> region, EXCHANGE or None (the checker then raises). A region is any hashable name of a part of the ring. ONCE is the region
# staged in the prologue and never refilled (the bias vector of the masked attention stream), EXCHANGE the area an epilogue writes
# with ds_write and reads back.
Layout = collections.namedtuple("Layout", "fill read")
ONCE, EXCHANGE = "staged once", "exchange"


def read_slot_from(s1):
    """address operand of a ds_read -> (kind, slot, k-step), for fragment addresses of slot 0 in %[fa0] %[fa1] %[fb0] %[fb1] and those of
    the other slots in v<s1>, v<s1 + 1> (A slot 1) and v<s1 + 2 slot>, v<s1 + 2 slot + 1> (B); None for any other operand"""
    def read_slot(a):
        if a.startswith("%[fa"):
            return "A", 0, int(a[4])
        if a.startswith("%[fb"):
            return "B", 0, int(a[4])
        r = int(a[1:]) - s1 if re.fullmatch(r"v\d+", a) else -1
        if r < 0:
            return None
        return ("A", 1, r) if r < 2 else ("B", r // 2, r % 2)
    return read_slot


def slot_layout(a_slots, a_bytes, b_bytes, s1):
    """the GEMM streams: a_slots activation slots of a_bytes, then the weight slots of b_bytes; regions (kind, slot)"""
    read_slot, b_base = read_slot_from(s1), a_slots * a_bytes

    def read(addr, off):
        slot = read_slot(addr)
        return slot and slot[:2]
    return Layout(lambda m0: ("A", m0 // a_bytes) if m0 < b_base else ("B", (m0 - b_base) // b_bytes), read)


def walk(lines, iterations):
    """prologue + iterations x loop body + exit, branches not taken"""
    try:
        i10, ibr = lines.index("10:"), lines.index("s_branch 10b")
    except ValueError as ex:
        raise WaitCoverageError("loop labels not found") from ex
    return lines[:i10] + lines[i10 + 1:ibr] * iterations + lines[ibr + 1:]


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


REGISTERS = re.compile(r"(?<![\w\[%])([av])(?:(\d+)|\[(\d+):(\d+)\])(?!\w)")   # v7, a[108:111]; not %[va0], 0xa0, vcc
LDS_READ = re.compile(r"ds_read_b\d+ (\S+), (\S+?)(?: offset:(\d+))?$")


def registers(text):
    """the VGPR / AGPR ranges an instruction names: [(file, first, last)]"""
    return [(f, int(one or lo), int(one or hi)) for f, one, lo, hi in REGISTERS.findall(text)]


def check_wait_coverage(lines, layout, iterations=3):
    """Static proof of the emitted stream's LDS ordering and register use. The waves of a workgroup run the same stream, so one wave's
    program order stands for all of them; the walk is prologue + iterations x loop body + exit with branches not taken. Every
    vector-memory instruction enters the in-order vmcnt queue, every LDS instruction (and the s_memtime of a --stamps build) the lgkmcnt
    queue; a counted s_waitcnt retires all but the newest N of its queue; an s_barrier behind the wait makes retired LDS-DMA fills
    `visible` and returned reads `fenced` for every wave. Then:
      RAW  a read of a ring region needs every LDS-DMA ever issued into the region to be visible;
      WAR  an LDS-DMA needs every earlier read of its region to be fenced (the region staged ONCE is never refilled behind a read);
           a ds_write needs that of every region and every fill to be visible; a read of the EXCHANGE area needs a ds_write before it;
      REG  no instruction names a VGPR / AGPR that overlaps the destination of an LDS read still in the lgkmcnt queue: an MFMA or
           VALU consumer ahead of its wait, or a ring entry reused before its previous read has returned.
    An LDS-DMA without m0, an LDS instruction `layout` cannot classify and a walk without ring traffic raise as well."""
    seq = walk(lines, iterations)
    vm, lg = [], []   # in issue order
    fills, reads = collections.defaultdict(list), collections.defaultdict(list)   # region -> operations (fills: all generations)
    m0, exchanged, n_reads, n_fills = None, False, 0, 0
    for pos, ins in enumerate(seq):
        if ins.startswith(";"):
            continue
        for f, lo, hi in registers(ins):
            for op in lg:
                if op["dst"] and op["dst"][0] == f and op["dst"][1] <= hi and lo <= op["dst"][2]:
                    raise WaitCoverageError(f"REG: `{ins}` at {pos} names a register of the LDS read at {op['pos']}, which is outstanding")
        mm = re.match(r"s_add_u32 m0, %\[wlds\], (\d+)", ins)
        if mm:
            m0 = int(mm.group(1))
        elif re.match(r"(buffer|global|flat|scratch)_(load|store|atomic)", ins):
            op = {"state": "inflight", "pos": pos}
            vm.append(op)
            if ins.endswith(" lds"):
                if m0 is None:
                    raise WaitCoverageError(f"LDS-DMA without an m0 destination at {pos}: {ins}")
                region = layout.fill(m0)
                for r in reads[region]:
                    if region == ONCE or r["state"] != "fenced":
                        raise WaitCoverageError(f"WAR: LDS-DMA into {region} at {pos} ({ins}) while the read of it at {r['pos']} is only "
                                                f"'{r['state']}' (needs an lgkmcnt wait and a barrier before the fill)")
                reads[region] = []
                fills[region].append(op)
                n_fills += region != ONCE
                m0 = None
        elif ins.startswith("ds_"):
            op = {"state": "issued", "pos": pos, "dst": None}
            mm = LDS_READ.match(ins)
            region = mm and layout.read(mm.group(2), int(mm.group(3) or 0))
            if mm and region == EXCHANGE:
                if not exchanged:
                    raise WaitCoverageError(f"exchange read at {pos} before any exchange write")
            elif mm and region is not None:
                if not fills[region]:
                    raise WaitCoverageError(f"RAW: ds_read of {region} at {pos} ({ins}) before anything was staged into it")
                for f in fills[region]:
                    if f["state"] != "visible":
                        raise WaitCoverageError(f"RAW: ds_read of {region} at {pos} ({ins}) while the LDS-DMA at {f['pos']} is only "
                                                f"'{f['state']}' (needs a covering vmcnt wait and a barrier before the read)")
                reads[region].append(op)
                n_reads += region != ONCE
            elif not mm and ins.startswith("ds_write"):
                busy = [(r, f) for r in fills for f in fills[r] if f["state"] != "visible"] + \
                       [(r, f) for r in reads for f in reads[r] if f["state"] != "fenced"]
                if busy:
                    region, f = busy[0]
                    raise WaitCoverageError(f"WAR: ds_write at {pos} while {region} is in use: the operation at {f['pos']} is only '{f['state']}'")
                exchanged = True
            else:
                raise WaitCoverageError(f"unclassified LDS instruction at {pos}: {ins}")
            if mm:
                op["dst"] = registers(mm.group(1))[0]
            lg.append(op)
        elif ins.startswith(("s_memtime", "s_load")):
            lg.append({"state": "issued", "pos": pos, "dst": None})
        elif ins.startswith("s_waitcnt"):
            vm = retire(vm, ins, "vmcnt", "retired")
            lg = retire(lg, ins, "lgkmcnt", "done")
        elif ins == "s_barrier":
            for ops, before, after in ((fills, "retired", "visible"), (reads, "done", "fenced")):
                for op in [op for region in ops for op in ops[region] if op["state"] == before]:
                    op["state"] = after
    if not n_reads or not n_fills:
        raise WaitCoverageError("checker saw no ring traffic - the stream format changed")
    return {"ring_reads": n_reads, "ring_fills": n_fills, "instructions": len(seq)}


# ---------------------------------------------------------------------------------------------------------------
# from a proven stream to the committed files
# ---------------------------------------------------------------------------------------------------------------
def finish(lines, save_m0, raw_race):
    """The asm block as the kernel includes it. m0 (the LDS-DMA destination) is a reserved register: naming it in the clobber list draws
    "-Winline-asm ... may lead to undefined behaviour" from the compiler, so the block saves it in an SGPR of its own and restores it on
    the way out; the surrounding HIP code sees m0 unchanged and the clobber list does not name it.
    Checker self-tests: --inject-raw-race replaces the loop's first `raw_race[0]` (the wait in front of a barrier that publishes staged
    tiles) by `raw_race[1]`, which leaves a part of a tile that is read next in flight; --inject-war-race drops the loop's first barrier."""
    lines = [f"s_mov_b32 s{save_m0}, m0"] + lines + [f"s_mov_b32 m0, s{save_m0}"]
    if "--inject-raw-race" in sys.argv:
        lines[lines.index(raw_race[0], lines.index("10:"))] = raw_race[1]
    if "--inject-war-race" in sys.argv:
        del lines[lines.index("s_barrier", lines.index("10:"))]
    return lines


def clobbers_inc(script, nv, na, sregs, part="main loop"):
    """v0 .. v<nv - 1>, a0 .. a<na - 1>, s<i> for i in sregs, twelve per line"""
    clob = [f"v{i}" for i in range(nv)] + [f"a{i}" for i in range(na)] + [f"s{i}" for i in sregs] + ["vcc", "scc", "memory"]
    text = f"// GENERATED by tools/{script} - do not edit. Registers the assembly {part} assigns by hand.\n"
    for i in range(0, len(clob), 12):
        text += ", ".join('"' + c + '"' for c in clob[i:i + 12]) + ("," if i + 12 < len(clob) else "") + "\n"
    return text


def emit(script, what, stem, diag, lines, stats, others, diag_status=4):
    """Writes csrc/<stem>.inc (the stream as string literals, headed "gfx950 assembly <what>") and `others` ({file name: text}), or with
    --check compares them with the committed files. A diagnostic build (`diag`: --stamps or schedule knobs) goes to <stem>_stamps.inc,
    which is not committed, and writes nothing else; --check of one exits with `diag_status` unless that file happens to be there."""
    text = f"// GENERATED by tools/{script} - do not edit. gfx950 assembly {what}.\n"
    text += "".join('"' + ln.replace('"', '\\"') + '\\n\\t"\n' for ln in lines)
    files = {stem + ("_stamps.inc" if diag else ".inc"): text}
    if "--check" in sys.argv or not diag:
        files.update(others)
    files = {os.path.join(CSRC, name): t for name, t in files.items()}
    if "--check" in sys.argv:
        same = all(os.path.exists(p) and open(p).read() == t for p, t in files.items())
        print(f"wait coverage ok: {stats}; committed output {'matches' if same else 'DIFFERS'}")
        sys.exit(0 if same else diag_status if diag else 4)
    for p, t in files.items():
        with open(p, "w") as f:
            f.write(t)
    if diag:
        print(f"{len(lines)} lines -> {os.path.normpath(next(iter(files)))}; {stats}")
    else:
        print(f"{len(lines)} lines, {sum(1 for ln in lines if 'v_mfma' in ln)} MFMAs; {stats}")
