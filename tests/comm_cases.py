"""The cases of tests/test_gpu_comm_operators.py, as data: which payloads the three collectives of the in-process
transport are fed, shared with tests/test_comm_ref.py, which shows on the CPU that every family below is needed to see
one of comm_ref.DEFECTS.

A SCENARIO is dict(name, world, steps): steps are collectives run back to back on one handle; a step is
  dict(kind="allreduce", rows (world, n), op, phase)
  dict(kind="allgatherv", offs (world + 1), rows (world, offs[-1]), phase)
  dict(kind="exchange", soffs, roffs (world lists of world + 1), send, recv (world arrays), send_phase, recv_phase)
FAMILIES maps a family's name to a function world -> list of scenarios (empty for a world the family does not use).
The shapes are the smallest at which each path of csrc/comm_kernels.hpp can go wrong: see the family's docstring.
"""
import numpy as np

import comm_ref as R

WORLDS = (2, 3, 8)
SENTINEL = np.array([0x7FF85E4711E15E47], dtype=np.uint64).view(np.float64)[0]  # "not this rank's to know" (a NaN)
ALLREDUCE_NS = (0, 1, 2, 3, 6, 7, 255, 256, 257, 513)
ALLREDUCE_LONG_N = 1024 * 256 + 3       # more than COMM_MAX_GRID_X x COMM_WG: k_comm_reduce's grid wraps
ALLGATHER_LONG_SPAN = 2 * 1024 * 256 + 3  # more than 2 x that: the copy's pair loop wraps


def spread(rng, shape):
    """seeded values over about 16 decades, both signs"""
    return rng.standard_normal(shape) * 10.0 ** rng.uniform(-8.0, 8.0, shape)


def special_columns(world, rng):
    """Columns (one double per rank) at which a wrong fold shows: the order of the additions, a NaN in a middle rank
    (not the last one: a max that loses it must meet a number after it), signed zeros, infinities, a denormal."""
    mid = (world - 1) // 2
    cols = []
    c = spread(rng, world)
    c[:min(world, 4)] = [1.0, 1e16, -1e16, 1.0][:min(world, 4)]  # ((1 + 1e16) - 1e16) + 1 = 1; any other order differs
    cols.append(c)
    c = spread(rng, world)
    c[mid] = np.nan
    cols.append(c)
    c = np.full(world, 0.0)
    c[0] = -0.0  # max keeps rank 0's -0.0 to the end (acc >= v holds for -0.0 >= +0.0); the sum is +0.0
    cols.append(c)
    c = spread(rng, world)
    c[world - 1] = np.inf
    cols.append(c)
    c = spread(rng, world)
    c[0] = -np.inf
    cols.append(c)
    c = spread(rng, world)
    c[:min(world, 3)] = [1e16, 1.0, -1e16][:min(world, 3)]
    cols.append(c)
    c = spread(rng, world) * 1e-300
    c[mid] = 5e-324
    cols.append(c)
    return cols


def operand_rows(world, n, seed):
    rng = np.random.default_rng(seed)
    rows = spread(rng, (world, n))
    for j, c in enumerate(special_columns(world, rng)):
        if j < n:
            rows[:, j] = c
    return rows


def payload(rng, n):
    """data of a copy: spread values with a few bit patterns a copy must not touch"""
    v = spread(rng, n)
    for j, x in enumerate((-0.0, np.nan, np.inf, 5e-324, -np.inf)):
        if 2 * j + 1 < n:
            v[2 * j + 1] = x
    return v


def one(name, world, step):
    return dict(name=name, world=world, steps=[step])


# ------------------------------------------------------------------------------------------------------ all-reduce
def allreduce_step(world, n, op, phase, seed):
    return dict(kind="allreduce", rows=operand_rows(world, n, seed), op=op, phase=phase)


def allreduce_small(world):
    """n around the head / pair / tail split and the workgroup size, both phases (phase 1: the put's scalar path, source
    and mailbox slot differ in phase), both ops.  Odd n: slots are `slot` = n + 1 apart, not n."""
    out = []
    for n in ALLREDUCE_NS:
        for phase in (0, 1):
            for op in (0, 1):
                out.append(one(f"allreduce n={n} phase={phase} op={op}", world,
                               allreduce_step(world, n, op, phase, 1000 + 10 * n + 2 * phase + op)))
    return out


def allreduce_long(world):
    """one n beyond COMM_MAX_GRID_X x COMM_WG on 3 ranks: k_comm_reduce's grid-stride loop goes round again (and, in
    phase 1, the put's scalar loop)"""
    if world != 3:
        return []
    return [one(f"allreduce long phase={phase} op={op}", world, allreduce_step(world, ALLREDUCE_LONG_N, op, phase, 77 + phase))
            for phase, op in ((0, 0), (1, 1))]


# ------------------------------------------------------------------------------------------------------ all-gather
def equal_plan(nb, world):
    """the engine's partition of nb block rows (partition_rows_equal), in doubles: 7 per row"""
    cnt = -(-nb // world)
    return [7 * min(r * cnt, nb) for r in range(world + 1)]


def allgather_plans(world):
    mid = world // 2
    cyc = [3, 2, 1, 7, 1, 2, 3, 9]
    plans = {
        "odd and even starts, spans of 1 2 3": np.cumsum([0] + {2: [3, 2], 3: [1, 2, 3]}.get(world, cyc[:world])),
        "empty first rank": np.cumsum([0, 0] + [cyc[r % 8] for r in range(1, world)]),
        "empty last rank": np.cumsum([0] + [cyc[r % 8] for r in range(world - 1)] + [0]),
        "one rank owns everything": np.cumsum([0] + [13 if r == mid else 0 for r in range(world)]),
        "engine's equal plan, short tail": np.array(equal_plan(2 * world - 1, world)),
        "more than one workgroup": np.cumsum([0] + [(513, 1030, 258)[r % 3] for r in range(world)]),
    }
    if world > 2:
        plans["empty middle rank"] = np.cumsum([0] + [0 if r == mid else cyc[r % 8] for r in range(world)])
    return {k: [int(x) for x in v] for k, v in plans.items()}


def allgather_step(world, offs, phase, seed):
    rng = np.random.default_rng(seed)
    rows = np.full((world, offs[-1]), SENTINEL)
    for r in range(world):
        rows[r, offs[r]:offs[r + 1]] = payload(rng, offs[r + 1] - offs[r])
    return dict(kind="allgatherv", offs=list(offs), rows=rows, phase=phase)


def allgather_small(world):
    """Phase 0 is comm_copy_span's pair path (vector and mailbox share the phase): a span that starts on an odd double has
    a head, one that ends on one a tail; spans of 1, 2 and 3 are a head alone, a pair alone or a tail alone, head + pair.
    Phase 1 is the scalar path.  Empty ranks: launches with fewer spans than peers, or none."""
    out = []
    for k, (name, offs) in enumerate(allgather_plans(world).items()):
        for phase in (0, 1):
            out.append(one(f"allgather {name} phase={phase}", world, allgather_step(world, offs, phase, 2000 + 2 * k + phase)))
    return out


def allgather_long(world):
    """one span of more than 2 x COMM_MAX_GRID_X x COMM_WG doubles on 2 ranks: the pair loop of the put (rank that owns
    it) and of the unpack (the other rank) goes round again -- from an even start, and from an odd one (a head first)"""
    if world != 2:
        return []
    L = ALLGATHER_LONG_SPAN
    return [one("allgather long span from an even double", 2, allgather_step(2, [0, L, L + 5], 0, 88)),
            one("allgather long span from an odd double", 2, allgather_step(2, [0, 1, L + 1], 0, 89))]


# -------------------------------------------------------------------------------------------------------- exchange
def exchange_step(world, counts, send_lead, recv_lead, send_phase, recv_phase, seed):
    """counts[p][q]: doubles rank p sends to rank q; *_lead[r]: where rank r's first segment starts in its buffer"""
    rng = np.random.default_rng(seed)
    counts = np.asarray(counts, dtype=np.int64)
    soffs = [[int(x) for x in send_lead[r] + np.concatenate([[0], np.cumsum(counts[r, :])])] for r in range(world)]
    roffs = [[int(x) for x in recv_lead[r] + np.concatenate([[0], np.cumsum(counts[:, r])])] for r in range(world)]
    send = [payload(rng, soffs[r][-1]) for r in range(world)]
    recv = [-(1000.0 * (r + 1) + np.arange(roffs[r][-1])) for r in range(world)]  # pre-fill: what a gap must keep
    return dict(kind="exchange", soffs=soffs, roffs=roffs, send=send, recv=recv, send_phase=send_phase,
                recv_phase=recv_phase)


def exchange_plans(world):
    lens = (0, 1, 2, 7, 9)
    mixed = [[lens[(3 * p + q) % 5] for q in range(world)] for p in range(world)]
    ring = np.zeros((world, world), dtype=np.int64)
    for p in range(world):
        ring[p][(p + 1) % world] = 7
    ring[1][0] += 9  # (world 2: rank 1 sends 16 to rank 0, rank 0 sends 7: both ways, unequal)
    one_way = np.zeros((world, world), dtype=np.int64)
    one_way[0][world - 1] = 9  # the last rank sends nothing to anybody
    return {"lengths 0 1 2 7 9, every pair": mixed, "most pairs empty": ring, "one pair, one way": one_way,
            "all empty": np.zeros((world, world), dtype=np.int64)}


def exchange_small(world):
    """Every combination of the two buffers' phases; segments of 0, 1, 2, 7 and 9 doubles that start on odd and on even
    doubles of their buffers (first segment at double r % 2 of the send, (r + 1) % 2 of the receive buffer), so that one
    launch has spans on the pair path and spans on the scalar path; the mailbox slots are even, so an odd length ends in
    a tail.  What lies in front of a receive buffer's first segment must keep its pre-fill."""
    out = []
    for k, (name, counts) in enumerate(exchange_plans(world).items()):
        for sp in (0, 1):
            for rp in (0, 1):
                out.append(one(f"exchange {name} send_phase={sp} recv_phase={rp}", world,
                               exchange_step(world, counts, [r % 2 for r in range(world)],
                                             [(r + 1) % 2 for r in range(world)], sp, rp, 3000 + 4 * k + 2 * sp + rp)))
    return out


# ---------------------------------------------------------------------------------------------------------- growth
def growth_counts(world, cap):
    """one rank's single segment is cap / world + 2 doubles (beyond the slot), every other segment at most 2"""
    counts = np.array([[(p + q) % 3 if p != q else 0 for q in range(world)] for p in range(world)], dtype=np.int64)
    counts[1, :] = 0
    counts[1][world - 1 if world > 2 else 0] = cap // world + 2
    return counts


def growth_step(world, cap, seed=4000):
    return exchange_step(world, growth_counts(world, cap), [0] * world, [0] * world, 0, 0, seed)


def growth_facts(step, world, cap):
    """the path condition on the plans and the capacity: who fits into the mailboxes as they are"""
    need = []
    for c in range(world):
        longest = max(max(step["soffs"][c][p + 1] - step["soffs"][c][p], step["roffs"][c][p + 1] - step["roffs"][c][p])
                      for p in range(world))
        need.append(world * ((longest + 1) & ~1))
    return dict(need=need, fits=[n <= cap for n in need])


GROWTH_MODEL_CAP = 64  # (what a first 1-double all-reduce leaves)


def growth(world):
    """an exchange in which ONE rank's segment does not fit: the ranks that fit put in round 0, the sender of the long
    segment and its receiver hold back, all grow, and round 1 repeats the collective; then the same exchange again"""
    if world == 2:
        return []
    step = growth_step(world, GROWTH_MODEL_CAP)
    return [dict(name="exchange that grows the mailboxes, twice", world=world, cap=GROWTH_MODEL_CAP,
                 steps=[step, growth_step(world, GROWTH_MODEL_CAP, 4001)])]


# ------------------------------------------------------------------------------------------------------- sequences
def sequence_steps(world, seed):
    """five collectives of mixed kind, lengths that shrink, other data each time: a mailbox read at the wrong parity, or
    not rewritten, leaves a value of an earlier collective where a later one is expected"""
    big = [int(x) for x in np.cumsum([0] + [9 + (r % 3) for r in range(world)])]
    small = [int(x) for x in np.cumsum([0] + [1 + (r % 2) if r < 3 else 0 for r in range(world)])]
    ring = np.zeros((world, world), dtype=np.int64)
    for p in range(world):
        ring[p][(p + 1) % world] = 9
        if world > 2:
            ring[(p + 1) % world][p] = 7
    return [allgather_step(world, big, 0, seed),
            exchange_step(world, ring, [0] * world, [0] * world, 0, 0, seed + 1),
            allreduce_step(world, 7, 0, 0, seed + 2),
            allgather_step(world, small, 1, seed + 3),
            allreduce_step(world, 2, 1, 1, seed + 4)]


def sequences(world):
    flip = allreduce_step(world, 1, 0, 0, 5555)
    return [dict(name="five collectives from an even count", world=world, start_parity=0, steps=sequence_steps(world, 5000)),
            dict(name="five collectives from an odd count", world=world, start_parity=1,
                 steps=[flip] + sequence_steps(world, 5100))]


FAMILIES = {"allreduce_small": allreduce_small, "allreduce_long": allreduce_long, "allgather_small": allgather_small,
            "allgather_long": allgather_long, "exchange_small": exchange_small, "growth": growth, "sequences": sequences}


def scenarios(family, worlds=WORLDS):
    return [s for w in worlds for s in FAMILIES[family](w)]


# ----------------------------------------------------------------------------------- one step, on anything that has them
def expected(step):
    if step["kind"] == "allreduce":
        return R.allreduce(list(step["rows"]), step["op"])
    if step["kind"] == "allgatherv":
        return R.allgatherv(step["offs"], list(step["rows"]))
    return R.exchange(step["soffs"], step["roffs"], step["send"], step["recv"])


def run_on_model(T, step):
    if step["kind"] == "allreduce":
        return T.allreduce(list(step["rows"]), step["op"], step["phase"])
    if step["kind"] == "allgatherv":
        return T.allgatherv(step["offs"], list(step["rows"]), step["phase"])
    return T.exchange(step["soffs"], step["roffs"], step["send"], step["recv"], step["send_phase"], step["recv_phase"])


def run_on_graph(G, step):
    """-> per-rank results of one sim3opt_comm_apply_* call on a set_devices graph"""
    if step["kind"] == "allreduce":
        return list(G.comm_apply_allreduce(step["rows"], step["op"], step["phase"]))
    if step["kind"] == "allgatherv":
        return list(G.comm_apply_allgatherv(step["offs"], step["rows"], step["phase"]))
    return G.comm_apply_exchange(step["soffs"], step["roffs"], step["send"], step["recv"], step["send_phase"],
                                 step["recv_phase"])
