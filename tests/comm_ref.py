"""Plain numpy restatements of the three collectives of the in-process transport (csrc/comm_local.hip,
csrc/comm_kernels.hpp), the yardstick of tests/test_gpu_comm_operators.py, and a MODEL of the transport itself that
tests/test_comm_ref.py uses to show that the yardstick and the cases of tests/comm_cases.py see defects.

The yardstick (allreduce, allgatherv, exchange) is index arithmetic and one fold on lists of per-rank float64 arrays:
  sum   ((s0 + s1) + s2) + ... in rank order, one float64 addition each
  max   acc if (acc >= v or acc != acc) else v, in rank order: a NaN wins, as in numpy.maximum (which
        dist_helpers.ThreadGroup.allreduce uses), and (-0.0, +0.0) keeps -0.0 (numpy.maximum leaves the sign of that zero
        to its vector path; the rule is the definition here, tests/test_comm_ref.py compares the two away from zeros)
Every comparison against it is on bits (bits()).

The model (Transport) walks what the device does: two alternating mailboxes per rank of one common capacity, operands
between guard doubles at an even or odd double of an aligned block, comm_copy_span's odd head / double2 pairs / odd tail
or its scalar path, the capped grids, the slots of the all-reduce and of the exchange, the second round of an exchange
that has to grow the mailboxes, and the collective count.  It remembers what the mailboxes last held, so defects that
read stale data can be restated.  With defect=None it must agree with the yardstick bit for bit on every case; each
name in DEFECTS switches one wrong behaviour on.
"""
import numpy as np

COMM_WG = 256
COMM_MAX_GRID_X = 1024
GUARD_DOUBLES = 4
GUARD = np.array([0x7FF4C0DEDBADF00D], dtype=np.uint64).view(np.float64)[0]   # what sim3opt_comm_apply_* writes
JUNK = np.array([0x7FF4000000BAD000], dtype=np.uint64).view(np.float64)[0]    # a mailbox double nobody has written

DEFECTS = ("fold_right", "fold_pairwise", "head_dropped", "tail_dropped", "pairs_one_short", "one_past", "slot_by_n",
           "max_loses_nan", "max_positive_zero", "other_parity", "old_slot_after_growth", "no_second_round_put",
           "one_sweep")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


# --------------------------------------------------------------------------------------------------- the yardstick
def maximum(acc, v, defect=None):
    with np.errstate(invalid="ignore"):
        if defect == "max_loses_nan":
            keep = acc >= v
        elif defect == "max_positive_zero":
            keep = (acc > v) | (acc != acc)
        else:
            keep = (acc >= v) | (acc != acc)
    return np.where(keep, acc, v)


def fold(rows, op, defect=None):
    """rows: per-rank float64 arrays of one length; op 0 sum, 1 max."""
    rows = [np.asarray(r, dtype=np.float64) for r in rows]

    def two(a, b):
        if op == 1:
            return maximum(a, b, defect)
        with np.errstate(invalid="ignore", over="ignore"):
            return a + b

    if defect == "fold_right":
        acc = rows[-1].copy()
        for r in rows[-2::-1]:
            acc = two(r, acc)
        return acc
    if defect == "fold_pairwise":
        lvl = [r.copy() for r in rows]
        while len(lvl) > 1:
            lvl = [two(lvl[i], lvl[i + 1]) if i + 1 < len(lvl) else lvl[i] for i in range(0, len(lvl), 2)]
        return lvl[0]
    acc = rows[0].copy()
    for r in rows[1:]:
        acc = two(acc, r)
    return acc


def allreduce(rows, op):
    """-> what every rank holds afterwards (a list of world equal arrays)"""
    res = fold(rows, op)
    return [res.copy() for _ in rows]


def allgatherv(offs, rows):
    """rows[r]: rank r's whole vector before; its span [offs[r], offs[r + 1]) is what the others get"""
    world = len(rows)
    out = []
    for r in range(world):
        v = np.array(rows[r], dtype=np.float64)
        for p in range(world):
            if p != r:
                v[offs[p]:offs[p + 1]] = rows[p][offs[p]:offs[p + 1]]
        out.append(v)
    return out


def exchange(soffs, roffs, send, recv):
    """soffs[r], roffs[r]: rank r's plan (world + 1 offsets each); recv[r]: its receive buffer before"""
    world = len(send)
    out = []
    for r in range(world):
        v = np.array(recv[r], dtype=np.float64)
        for p in range(world):
            n = roffs[r][p + 1] - roffs[r][p]
            assert n == soffs[p][r + 1] - soffs[p][r], "the plans disagree"
            v[roffs[r][p]:roffs[r][p + 1]] = send[p][soffs[p][r]:soffs[p][r + 1]]
        out.append(v)
    return out


# ------------------------------------------------------------------------------------------- the device, restated
def copy_grid(nmax):
    """launch_spans: workgroups in x for the longest span of a launch"""
    return min(COMM_MAX_GRID_X, max(1, (nmax // 2 + COMM_WG - 1) // COMM_WG))


def reduce_grid(n):
    return min(COMM_MAX_GRID_X, max(1, (n + COMM_WG - 1) // COMM_WG))


def span_path(dst_index, src_index, n, gx):
    """What comm_copy_span does with one span whose first double sits at these (absolute, 16-byte aligned base) indices:
    dict(same_phase, head, pairs, tail, sweeps) -- the path conditions the GPU test asserts from its inputs."""
    nt = gx * COMM_WG
    same = ((dst_index ^ src_index) & 1) == 0
    if not same:
        return dict(same_phase=False, head=0, pairs=0, tail=0, sweeps=-(-n // nt))
    head = 1 if (dst_index & 1) and n > 0 else 0
    pairs = (n - head) // 2
    return dict(same_phase=True, head=head, pairs=pairs, tail=1 if head + 2 * pairs < n else 0, sweeps=-(-pairs // nt))


def copy_span(dst, d0, src, s0, n, gx, defect=None):
    """comm_copy_span on arrays whose index parity is the address's 16-byte phase"""
    if n <= 0:
        return
    nt = gx * COMM_WG
    p = span_path(d0, s0, n, gx)
    if not p["same_phase"]:
        m = min(n, nt) if defect == "one_sweep" else n
        dst[d0:d0 + m] = src[s0:s0 + m]
    else:
        head, pairs = p["head"], p["pairs"]
        if head and defect != "head_dropped":
            dst[d0] = src[s0]
        done = pairs
        if defect == "pairs_one_short":
            done = max(pairs - 1, 0)
        if defect == "one_sweep":
            done = min(pairs, nt)
        dst[d0 + head:d0 + head + 2 * done] = src[s0 + head:s0 + head + 2 * done]
        if p["tail"] and defect != "tail_dropped":
            dst[d0 + n - 1] = src[s0 + n - 1]
    if defect == "one_past" and d0 + n < len(dst):
        dst[d0 + n] = src[s0 + n] if s0 + n < len(src) else 0.0


class Operand:
    """A rank's operand as sim3opt_comm_apply_* holds it: guards, `phase` more of them, the data, guards."""

    def __init__(self, data, phase):
        data = np.asarray(data, dtype=np.float64)
        self.lead, self.n = GUARD_DOUBLES + phase, len(data)
        self.a = np.full(self.lead + self.n + GUARD_DOUBLES, GUARD)
        self.a[self.lead:self.lead + self.n] = data

    def data(self):
        return self.a[self.lead:self.lead + self.n].copy()

    def guards_ok(self):
        g = np.concatenate([self.a[:self.lead], self.a[self.lead + self.n:]])
        return bool((bits(g) == bits(GUARD)).all())


class Transport:
    """The ranks' mailboxes, their capacity and the collective count, from one collective to the next."""

    def __init__(self, world, cap=0, seq=0, defect=None):
        assert defect is None or defect in DEFECTS, defect
        self.world, self.cap, self.seq, self.defect = world, cap, seq, defect
        self.mbox = [[np.full(cap, JUNK), np.full(cap, JUNK)] for _ in range(world)]
        self.guards_ok = True

    # -- comm_local.hip
    def _ensure(self, need):
        if need <= self.cap:
            return False
        cap = max(self.cap, 64)
        while cap < need:
            cap *= 2
        self.cap = cap
        self.mbox = [[np.full(cap, JUNK), np.full(cap, JUNK)] for _ in range(self.world)]
        self.seq += 1
        return True

    def _launch(self, spans):
        """one k_comm_put / k_comm_unpack: spans of (dst array, dst index, src array, src index, n)"""
        spans = [s for s in spans if s[4] > 0]
        if not spans:
            return
        gx = copy_grid(max(s[4] for s in spans))
        for dst, d0, src, s0, n in spans:
            copy_span(dst, d0, src, s0, n, gx, self.defect)

    def _read_parity(self, par):
        return par ^ 1 if self.defect == "other_parity" else par

    def _note(self, ops):
        self.guards_ok = self.guards_ok and all(o.guards_ok() for o in ops)

    def allreduce(self, rows, op, phase=0):
        world, n = self.world, len(rows[0])
        ops = [Operand(r, phase) for r in rows]
        slot = (n + 1) & ~1
        self._ensure(slot * world)
        par = self.seq & 1
        for c in range(world):
            self._launch([(self.mbox[p][par], slot * c, ops[c].a, ops[c].lead, n) for p in range(world)])
        self.seq += 1
        stride = n if self.defect == "slot_by_n" else slot
        m = min(n, reduce_grid(n) * COMM_WG) if self.defect == "one_sweep" else n
        for c in range(world):
            mb = self.mbox[c][self._read_parity(par)]
            res = fold([mb[r * stride:r * stride + n] for r in range(world)], op, self.defect)
            ops[c].a[ops[c].lead:ops[c].lead + m] = res[:m]
        self._note(ops)
        return [o.data() for o in ops]

    def allgatherv(self, offs, rows, phase=0):
        world, total = self.world, int(offs[-1])
        ops = [Operand(r, phase) for r in rows]
        self._ensure(total)
        par = self.seq & 1
        for c in range(world):
            lo, hi = int(offs[c]), int(offs[c + 1])
            self._launch([(self.mbox[p][par], lo, ops[c].a, ops[c].lead + lo, hi - lo) for p in range(world) if p != c])
        self.seq += 1
        for c in range(world):
            lo, hi = int(offs[c]), int(offs[c + 1])
            mb, o = self.mbox[c][self._read_parity(par)], ops[c]
            self._launch([(o.a, o.lead, mb, 0, lo), (o.a, o.lead + hi, mb, hi, total - hi)])
        self._note(ops)
        return [o.data() for o in ops]

    def exchange(self, soffs, roffs, send, recv, send_phase=0, recv_phase=0):
        world = self.world
        sops = [Operand(s, send_phase) for s in send]
        rops = [Operand(r, recv_phase) for r in recv]
        need = [world * ((max(max(soffs[c][p + 1] - soffs[c][p], roffs[c][p + 1] - roffs[c][p]) for p in range(world)) + 1)
                         & ~1) for c in range(world)]
        fitted, old_slot = [False] * world, None
        for rnd in range(2):
            par = self.seq & 1
            slot = (self.cap // world) & ~1
            for c in range(world):
                fits = need[c] <= self.cap
                if rnd == 0:
                    fitted[c] = fits
                if fits and not (rnd == 1 and fitted[c] and self.defect == "no_second_round_put"):
                    self._launch([(self.mbox[p][par], slot * c, sops[c].a, sops[c].lead + soffs[c][p],
                                   soffs[c][p + 1] - soffs[c][p]) for p in range(world)])
            self.seq += 1
            if max(need) > self.cap:  # (every rank sees every request after the barrier: all grow, and go round again)
                assert rnd == 0
                old_slot = slot
                self._ensure(max(need))
                continue
            if rnd == 1 and self.defect == "old_slot_after_growth":
                slot = old_slot
            for c in range(world):
                mb = self.mbox[c][self._read_parity(par)]
                self._launch([(rops[c].a, rops[c].lead + roffs[c][p], mb, slot * p, roffs[c][p + 1] - roffs[c][p])
                              for p in range(world)])
            break
        self._note(sops + rops)
        return [o.data() for o in rops]
