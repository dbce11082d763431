"""The contract of bl_amd_desc_chain_* (include/bliss_amd.h) in numpy int64 and Python integers: chains over
descriptors under the mix rules, nearest = the smallest (d2, index).  The chains of a call are walked in lockstep in
groups of 16, as the kernels walk them, which changes no result (chains are independent) but lets the switches below
make the mistakes such a kernel could make.

`bugs` is a set of switches that make plausible mistakes on purpose, so that the tests can show that their cases tell
the contract from each of them (tests/test_desc_chain_reference_host.py):

  tie_larger           a tie in d2 goes to the larger index
  forget_played        the pick's bit is not set
  seed_not_played      the index seed is not marked played
  exclude_blocks_seed  an excluded index seed is replaced (by the nearest song not excluded) instead of taking slot 0
  gap_off_by_one       the gap window is one slot off: the tag of slot t - gap - 1 still blocks at slot t
  negative_tag_blocks  an untagged song is blocked by an equal negative tag in the window
  seed_desc_tags       a tag blocks slot 0 of a descriptor seed: the window starts with the tag of song 0
  value_from_seed      d2 is measured from slot 0 instead of slot t - 1
  shared_played        the chains of a group share one played set
  row_swap             chain r advances from chain r ^ 1's current song
  end_continues        a chain with no allowed song goes on with a disallowed one (the nearest unplayed)

cases() are the named inputs the GPU tests run, and SWITCH_CASE names, for every switch, a case and a row of it that
the switch changes."""
import numpy as np

from tests.desc_reference import DIMS, EMPTY, IDX_BITS, SCALE_MAX, d2_direct, one_hot_sets

GROUP = 16
MAX_GAP = 16
BUGS = ("tie_larger", "forget_played", "seed_not_played", "exclude_blocks_seed", "gap_off_by_one",
        "negative_tag_blocks", "seed_desc_tags", "value_from_seed", "shared_played", "row_swap", "end_continues")


def _nearest(d2, allowed, bugs):
    """(index, d2) of the allowed candidate with the smallest (d2, index), or None"""
    if not allowed.any():
        return None
    idx = np.arange(d2.size, dtype=np.uint64)
    low = (np.uint64(2 ** IDX_BITS - 1) - idx) if "tie_larger" in bugs else idx
    keys = np.where(allowed, (d2.astype(np.uint64) << np.uint64(IDX_BITS)) | low, np.uint64(EMPTY))
    j = int(np.argmin(keys))
    return j, int(d2[j])


def chain(lib, seeds=None, length=1, tags=None, gap=0, exclude=None, seed_desc=None, bugs=()):
    """(order int32 (n_chains, length), dist2 uint64 (n_chains, length)) of the device forms: a seed outside [0, n)
    gives a row of -1 / 2^64 - 1"""
    bugs = set(bugs)
    assert not bugs - set(BUGS)
    lib = np.asarray(lib)
    n = lib.shape[0]
    assert 1 <= n < 2 ** IDX_BITS and lib.shape[1] == DIMS and length >= 1 and 0 <= gap <= MAX_GAP
    assert (seeds is None) != (seed_desc is None) and (gap == 0 or tags is not None)
    seeds = None if seeds is None else [int(s) for s in np.asarray(seeds).reshape(-1)]
    seed_desc = None if seed_desc is None else np.asarray(seed_desc)
    n_chains = len(seeds) if seeds is not None else seed_desc.shape[0]
    ex = np.zeros(n, dtype=bool) if exclude is None else np.asarray(exclude).astype(bool)
    tg = None if gap == 0 else np.asarray(tags).astype(np.int64)
    order = np.full((n_chains, length), -1, dtype=np.int32)
    dist2 = np.full((n_chains, length), EMPTY, dtype=np.uint64)
    steps = min(length, n)
    for g0 in range(0, n_chains, GROUP):
        rows = list(range(g0, min(g0 + GROUP, n_chains)))
        shared = np.zeros(n, dtype=bool)
        played = {c: (shared if "shared_played" in bugs else np.zeros(n, dtype=bool)) for c in rows}
        slot_tags = {c: {} for c in rows}   # slot -> tag of its song
        query = {}                          # the vector the next slot is measured from
        first = {}                          # the vector of slot 0 (value_from_seed)
        alive = {c: True for c in rows}
        t0 = 1
        for c in rows:
            if seeds is None:
                query[c] = first[c] = seed_desc[c]
                t0 = 0
                if "seed_desc_tags" in bugs and tg is not None:
                    slot_tags[c][-1] = int(tg[0])
                continue
            s = seeds[c]
            if not 0 <= s < n:
                alive[c] = False
                continue
            if "exclude_blocks_seed" in bugs and ex[s]:
                hit = _nearest(d2_direct(lib[s][None], lib)[0], ~ex, bugs)
                if hit is None:
                    alive[c] = False
                    continue
                s, v = hit
                order[c, 0], dist2[c, 0] = s, v
            else:
                order[c, 0], dist2[c, 0] = s, 0
            query[c] = first[c] = lib[s]
            if "seed_not_played" not in bugs:
                played[c][s] = True
            if tg is not None:
                slot_tags[c][0] = int(tg[s])
        for t in range(t0, steps):
            picks = {}
            for c in rows:
                if not alive[c]:
                    continue
                src = c
                if "row_swap" in bugs and (c ^ 1) in query and alive.get(c ^ 1, False):
                    src = c ^ 1
                d2 = d2_direct(np.asarray(query[src])[None], lib)[0]
                allowed = ~played[c] & ~ex
                if tg is not None:
                    width = gap + 1 if "gap_off_by_one" in bugs else gap
                    window = [slot_tags[c][u] for u in range(t - width, t) if u in slot_tags[c]]
                    for w in set(window):
                        if w >= 0 or "negative_tag_blocks" in bugs:
                            allowed &= tg != w
                hit = _nearest(d2, allowed, bugs)
                if hit is None and "end_continues" in bugs:
                    hit = _nearest(d2, ~played[c], bugs)
                if hit is None:
                    alive[c] = False
                    continue
                j, v = hit
                if "value_from_seed" in bugs:
                    v = int(d2_direct(np.asarray(first[c])[None], lib[j][None])[0, 0])
                picks[c] = (j, v)
            for c, (j, v) in picks.items():   # lockstep: the step's picks take effect together
                order[c, t], dist2[c, t] = j, v
                query[c] = lib[j]
                if "forget_played" not in bugs:
                    played[c][j] = True
                if tg is not None:
                    slot_tags[c][t] = int(tg[j])
    return order, dist2


def brute(lib, seed, length, tags=None, gap=0, exclude=None, seed_vec=None):
    """One chain by the header's sentences, in plain Python integers: [(song, d2)] of the slots it fills"""
    lib = [[int(x) for x in row] for row in np.asarray(lib)]
    n = len(lib)
    dist = lambda a, b: sum((x - y) ** 2 for x, y in zip(a, b))
    out = []
    if seed_vec is None:
        if not 0 <= seed < n:
            return out
        out.append((seed, 0))
    else:
        cand = [(dist([int(x) for x in seed_vec], lib[j]), j) for j in range(n) if not (exclude is not None and exclude[j])]
        if not cand:
            return out
        d, j = min(cand)
        out.append((j, d))
    for t in range(1, min(length, n)):
        prev = lib[out[t - 1][0]]
        cand = []
        for j in range(n):
            if any(j == s for s, _ in out) or (exclude is not None and exclude[j]):
                continue
            if gap > 0 and tags[j] >= 0 and any(tags[out[u][0]] == tags[j] for u in range(max(0, t - gap), t)):
                continue
            cand.append((dist(prev, lib[j]), j))
        if not cand:
            break
        d, j = min(cand)
        out.append((j, d))
    return out


# ---------------------------------------------------------------------------
# libraries and the named cases of the GPU tests

def random_lib(n, seed):
    """full scale: |q| up to 32512, d2 up to 2^37"""
    rng = np.random.default_rng(seed)
    lib = rng.integers(-SCALE_MAX, SCALE_MAX + 1, size=(n, DIMS)).astype(np.int16)
    lib[rng.integers(0, n)] = SCALE_MAX
    lib[rng.integers(0, n)] = -SCALE_MAX
    return lib


def tie_lib(n, seed):
    """entries from {-1, 0, 1} in two columns: nine distinct descriptors, so nearly every step is decided by the index"""
    rng = np.random.default_rng(seed)
    lib = np.zeros((n, DIMS), dtype=np.int16)
    lib[:, 3] = rng.integers(-1, 2, size=n)
    lib[:, 20] = rng.integers(-1, 2, size=n)
    return lib


def cases():
    """name -> keyword arguments of chain()"""
    out = {}
    rng = np.random.default_rng(1234)
    # plain chains over a tie-heavy library, more than two groups, ties across tiles and waves
    out["ties"] = dict(lib=tie_lib(257, 1), seeds=rng.integers(0, 257, size=33).astype(np.int32), length=24)
    # full-scale values, every rule at once: an excluded seed, untagged songs, two groups, length past n
    lib = random_lib(33, 2)
    tags = rng.integers(0, 5, size=33).astype(np.int32)
    tags[rng.random(33) < 0.3] = -1
    tags[[0, 1, 2]] = [-1, -7, -7]
    ex = rng.random(33) < 0.2
    ex[5] = True
    seeds = np.arange(17, dtype=np.int32)
    seeds[3] = 5
    out["rules"] = dict(lib=lib, seeds=seeds, length=36, tags=tags, gap=2, exclude=ex)
    # two tags only and gap 1: a chain must alternate and ends when one tag runs out, at different slots per row
    lib = random_lib(40, 3)
    tags = (rng.random(40) < 0.3).astype(np.int32)
    out["two_tags"] = dict(lib=lib, seeds=np.arange(0, 34, 2, dtype=np.int32), length=40, tags=tags, gap=1)
    # descriptor seeds: one equal to a library song, the rest from outside; tags and a mask
    lib = random_lib(65, 4)
    sd = random_lib(18, 5)
    sd[4] = lib[7]
    tags = rng.integers(0, 3, size=65).astype(np.int32)
    ex = rng.random(65) < 0.1
    ex[7] = False
    out["seed_desc"] = dict(lib=lib, seed_desc=sd, length=20, tags=tags, gap=16, exclude=ex)
    # the tile layout: one-hot descriptors with distinct digits
    a, b = one_hot_sets()
    out["one_hot"] = dict(lib=np.concatenate([a, b]), seeds=np.arange(64, dtype=np.int32)[::3], length=64)
    return out


# switch -> (case, row): the row of the case's output that the switch changes
SWITCH_CASE = {
    "tie_larger": ("ties", 0),
    "forget_played": ("ties", 1),
    "seed_not_played": ("ties", 3),
    "shared_played": ("ties", 20),
    "row_swap": ("ties", 29),
    "value_from_seed": ("rules", 0),
    "exclude_blocks_seed": ("rules", 3),
    "gap_off_by_one": ("rules", 1),
    "negative_tag_blocks": ("rules", 2),
    "end_continues": ("two_tags", 0),
    "seed_desc_tags": ("seed_desc", 4),
}
