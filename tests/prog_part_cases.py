"""Shared by tests/test_prog_part_host.py and tests/test_gpu_prog_stepper.py: the shard splits of
tests/prog_cases.select_cases() and helpers around the shard-partial record (csrc/prog_rule.h,
include/maxcover.h mac_prog_part)."""
import struct

import numpy as np

import prog_cases as pc

WORLDS = (1, 2, 3, 8)
_cache = {}


def edges(K):
    """The shard edges the splits draw from: the wave and block sizes of prog_part_kernel and their
    neighbours, the ends of the poll."""
    return sorted({e for e in (0, 1, 63, 64, 65, 255, 256, 257, K - 1, K) if 0 <= e <= K})


def split(K, P, rng):
    """P contiguous shards [(lo, hi)] that partition [0, K), their cuts drawn from edges(K) (repeats
    give empty shards, and for P >= 2 one cut is repeated on purpose: at least one shard is empty),
    returned in a shuffled order: the order the records are merged in."""
    if P == 1:
        return [(0, K)]
    cuts = list(rng.choice(edges(K), P - 2)) if P > 2 else []
    cuts.append(int(rng.choice(cuts + [0, K])))   # a repeated cut: an empty shard
    cuts = [0] + sorted(int(c) for c in cuts) + [K]
    shards = [(cuts[q], cuts[q + 1]) for q in range(P)]
    assert any(lo == hi for lo, hi in shards) and sum(hi - lo for lo, hi in shards) == K
    return [shards[q] for q in rng.permutation(P)]


def split_cases():
    """[(case, want, [shards for P in WORLDS])] over select_cases(), the same on every call. want: the
    hand-written cases' own answer, else select_written_out's."""
    if "splits" not in _cache:
        rng = np.random.default_rng(20250301)
        out = []
        for case in pc.select_cases():
            want = case["want"]
            if want is None:
                want = pc.select_written_out(*pc.rule_args(case), case["obj"], case["h"], case["K"])
            out.append((case, want, [split(case["K"], P, rng) for P in WORLDS]))
        _cache["splits"] = out
    return _cache["splits"]


def shard_cands(case, lo, hi):
    """[(f, h, g)] of the shard [lo, hi) of every polled centre, g = centre K + k."""
    K = case["K"]
    out = []
    for c in (0, 1):
        if case["obj"][c] is None:
            continue
        out += [(float(case["obj"][c][k]), float(case["h"][c][k]), c * K + k) for k in range(lo, hi)]
    return out


def part_bytes(part):
    """A record (a 12-tuple in mac_prog_part's field order, or a ctypes ProgPart) as its 96 bytes."""
    if not isinstance(part, tuple):
        return bytes(part)
    t = part
    return struct.pack("<qqdqqdddqddq", int(t[0]), int(t[1]), float(t[2]), int(t[3]), int(t[4]),
                       float(t[5]), float(t[6]), float(t[7]), int(t[8]), float(t[9]), float(t[10]), int(t[11]))


def chains_written_out(rec, has_I):
    """Whether the iteration was unsuccessful and left I as it was: by the definition, on ProgRec's fields."""
    unsuccessful = (rec[0] & 255) == 2
    same_I = rec[5] == pc.NEW_I_OLD or (not has_I and rec[5] == pc.NEW_I_NONE)
    return unsuccessful and same_I


# ---------------------------------------------------------------- several steppers in one process

class LocalGather:
    """The exchange among prog steppers of one process: "rank" j's record from its own poll (ahead=True:
    rank j polls j iterations ahead, the speculative loop)."""

    def __init__(self, others, ahead=False):
        self.others, self.rank, self.world, self.ahead = others, 0, len(others) + 1, ahead

    def __call__(self, part):
        return [part] + [s.poll(j + 1 if self.ahead else 0)[1] for j, s in enumerate(self.others)]


def lock_step(steppers, loop, ahead=False):
    """``loop`` (dist.mads_prog_loop or dist.mads_prog_loop_speculative) on steppers[0], the others polled
    beside it and advanced with every record it applies. Returns (the loop's result, records applied per
    exchange)."""
    lead, others = steppers[0], steppers[1:]
    adv, poll = lead.advance, lead.poll
    rounds = []

    def advance_all(part):
        for s in others:
            s.advance(part)
        rounds[-1] += 1
        return adv(part)

    def poll_counted(a=0):
        rounds.append(0)
        return poll(a)

    lead.advance, lead.poll = advance_all, poll_counted
    try:
        res = loop(lead, LocalGather(others, ahead) if others else None)
    finally:
        del lead.advance, lead.poll
    return res, rounds


def rounds_written_out(outcomes_and_I, had_I, world):
    """The iterations each speculative exchange applies, from the sequential run's per-iteration
    (outcome, I exists afterwards): an exchange applies up to ``world`` iterations and stops after the
    first that is not unsuccessful or that changes whether I exists."""
    chain = []
    for outcome, has_I in outcomes_and_I:
        chain.append(outcome == "unsuccessful" and has_I == had_I)
        had_I = has_I
    want, q = [], 0
    while q < len(chain):
        n = 1
        while n < world and chain[q + n - 1] and q + n < len(chain):
            n += 1
        want.append(n)
        q += n
    return want
