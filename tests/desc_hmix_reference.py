"""The contract of bl_amd_desc_hmix_* (include/bliss_amd.h) in numpy int64 and Python integers: the chains of
tests/desc_chain_reference.py under one more rule, on the pair (song of slot t - 1, candidate).  Slot 0, the distances,
the order of candidates and the libraries come from that module; what is written here is the pair rule and a walker
that applies it beside the mask, the played set and the tags.  The chains of a call are walked in lockstep in groups of
16, as the kernels walk them, so that the switches below can make the mistakes such a kernel could make.

attrs is an (n, 2) integer array, (tempo in 1/100 BPM, key); rule a dict with key_ok (24 integers), tempo_tol, flags.

`bugs` is a set of switches (tests/test_desc_hmix_reference_host.py shows that each changes a named row of a case):

  table_transposed          bit ka of key_ok[kb] is tested
  tol_of_candidate          the tolerance is taken of the candidate's tempo
  unknown_key_blocks        an unknown key on either side blocks
  unknown_tempo_blocks      an unknown tempo on either side blocks
  key_ge_24_indexes_table   a key >= 24 is reduced mod 24 and looked up like a known one
  rule_from_slot0           the attribute is not refreshed after a pick: every slot is tested against slot 0's song
  row_swap_attr             row r tests against row r ^ 1's previous song
  half_only                 double time is not matched
  double_tol_not_doubled    `tol a` in place of `2 tol a` in the double-time inequality
  blocked_lowers_bound      a blocked candidate nearer than every allowed one ends the step empty
  seed_desc_ruled           slot 0 of a descriptor seed is tested against song 0's attribute
  seed_attr_ignored         an index seed's attribute does not bind slot 1

cases() are the named inputs the GPU tests run, and SWITCH_CASE names a case and a row per switch."""
import numpy as np

from tests import desc_chain_reference as R
from tests.desc_reference import EMPTY, d2_direct

KEY, TEMPO, HALF_DOUBLE = 1, 2, 4
BUGS = ("table_transposed", "tol_of_candidate", "unknown_key_blocks", "unknown_tempo_blocks",
        "key_ge_24_indexes_table", "rule_from_slot0", "row_swap_attr", "half_only", "double_tol_not_doubled",
        "blocked_lowers_bound", "seed_desc_ruled", "seed_attr_ignored")


def camelot(tempo_tol, flags):
    """the wheel of bl_amd_hmix_rule_camelot, from the header's formula"""
    table = [0] * 24
    for k in range(12):
        table[k] = 1 << k | 1 << (k + 7) % 12 | 1 << (k + 5) % 12 | 1 << 12 + (k + 9) % 12
        table[12 + k] = 1 << 12 + k | 1 << 12 + (k + 7) % 12 | 1 << 12 + (k + 5) % 12 | 1 << (k + 3) % 12
    return dict(key_ok=table, tempo_tol=tempo_tol, flags=flags)


def rule_ok(rule):
    f, tol = rule["flags"], rule["tempo_tol"]
    return not f & ~7 and not (f & HALF_DOUBLE and not f & TEMPO) and 0 <= tol <= 1000 and len(rule["key_ok"]) == 24


def pair_ok(prev, attrs, rule, bugs=()):
    """bool (n,): which songs pass against a previous song of attribute prev = (tempo, key)"""
    a, ka = int(prev[0]), int(prev[1])
    b, kb = attrs[:, 0].astype(np.int64), attrs[:, 1].astype(np.int64)
    table = np.array([int(x) & 0xFFFFFF for x in rule["key_ok"]], dtype=np.int64)
    tol, flags = int(rule["tempo_tol"]), int(rule["flags"])
    ok = np.ones(attrs.shape[0], dtype=bool)
    if flags & KEY:
        known = (kb < 24) & (ka < 24)
        if "key_ge_24_indexes_table" in bugs:
            known = np.ones_like(known)
        ia, ib = ka % 24, kb % 24
        bit = (table[ib] >> ia) & 1 if "table_transposed" in bugs else (table[ia] >> ib) & 1
        ok &= np.where(known, bit == 1, "unknown_key_blocks" not in bugs)
    if flags & TEMPO:
        base = b if "tol_of_candidate" in bugs else a
        hit = 1000 * np.abs(b - a) <= tol * base
        if flags & HALF_DOUBLE:
            hit |= 1000 * np.abs(2 * b - a) <= tol * base
            if "half_only" not in bugs:
                hit |= 1000 * np.abs(b - 2 * a) <= (1 if "double_tol_not_doubled" in bugs else 2) * tol * base
        ok &= np.where((b != 0) & (a != 0), hit, "unknown_tempo_blocks" not in bugs)
    return ok


def hmix(lib, attrs, rule, seeds=None, length=1, tags=None, gap=0, exclude=None, seed_desc=None, bugs=()):
    """(order int32 (n_chains, length), dist2 uint64 (n_chains, length)) of the device forms"""
    bugs = set(bugs)
    assert not bugs - set(BUGS) and rule_ok(rule)
    lib = np.asarray(lib)
    n = lib.shape[0]
    ruled = bool(rule["flags"] & (KEY | TEMPO))
    attrs = np.zeros((n, 2), dtype=np.int64) if attrs is None else np.asarray(attrs).astype(np.int64)
    assert attrs.shape == (n, 2)
    ex = np.zeros(n, dtype=bool) if exclude is None else np.asarray(exclude).astype(bool)
    tg = None if gap == 0 else np.asarray(tags).astype(np.int64)
    # slot 0 is the chain's
    first = R.chain(lib, seeds=seeds, length=1, tags=tags, gap=gap, exclude=exclude, seed_desc=seed_desc)
    n_chains = first[0].shape[0]
    order = np.full((n_chains, length), -1, dtype=np.int32)
    dist2 = np.full((n_chains, length), EMPTY, dtype=np.uint64)
    order[:, 0], dist2[:, 0] = first[0][:, 0], first[1][:, 0]
    if seed_desc is not None and ruled and "seed_desc_ruled" in bugs:
        for c in range(n_chains):
            d2 = d2_direct(np.asarray(seed_desc)[c][None], lib)[0]
            hit = R._nearest(d2, ~ex & pair_ok(attrs[0], attrs, rule), ())
            order[c, 0], dist2[c, 0] = (-1, EMPTY) if hit is None else hit
    for g0 in range(0, n_chains, R.GROUP):
        rows = list(range(g0, min(g0 + R.GROUP, n_chains)))
        played = {c: np.zeros(n, dtype=bool) for c in rows}
        alive = {c: order[c, 0] >= 0 for c in rows}
        for c in rows:
            if alive[c]:
                played[c][order[c, 0]] = True
        for t in range(1, min(length, n)):
            picks = {}
            for c in rows:
                if not alive[c]:
                    continue
                p = int(order[c, t - 1])
                allowed = ~played[c] & ~ex
                if tg is not None:
                    for u in range(max(0, t - gap), t):
                        w = tg[order[c, u]]
                        if w >= 0:
                            allowed &= tg != w
                src = c ^ 1 if "row_swap_attr" in bugs and alive.get(c ^ 1, False) else c
                q = int(order[src, 0 if "rule_from_slot0" in bugs else t - 1])
                ok = pair_ok(attrs[q], attrs, rule, bugs)
                if not ruled or ("seed_attr_ignored" in bugs and t == 1 and seeds is not None):
                    ok = np.ones(n, dtype=bool)
                d2 = d2_direct(lib[p][None], lib)[0]
                hit = R._nearest(d2, allowed & ok, ())
                if "blocked_lowers_bound" in bugs:
                    near = R._nearest(d2, allowed, ())
                    if near is not None and not ok[near[0]]:
                        hit = None
                if hit is None:
                    alive[c] = False
                else:
                    picks[c] = hit
            for c, (j, v) in picks.items():   # lockstep: the step's picks take effect together
                order[c, t], dist2[c, t] = j, v
                played[c][j] = True
    return order, dist2


def brute(lib, attrs, rule, seed, length, tags=None, gap=0, exclude=None, seed_vec=None):
    """One chain by the header's sentences, in plain Python integers: [(song, d2)] of the slots it fills"""
    lib = [[int(x) for x in row] for row in np.asarray(lib)]
    n = len(lib)
    at = [(int(t), int(k)) for t, k in np.asarray(attrs)] if attrs is not None else [(0, 255)] * n
    table, tol, flags = [int(x) for x in rule["key_ok"]], int(rule["tempo_tol"]), int(rule["flags"])
    dist = lambda x, y: sum((p - q) ** 2 for p, q in zip(x, y))
    masked = lambda j: exclude is not None and bool(exclude[j])

    def passes(p, j):
        (a, ka), (b, kb) = at[p], at[j]
        if flags & KEY and not (ka >= 24 or kb >= 24 or table[ka] >> kb & 1):
            return False
        if flags & TEMPO and not (a == 0 or b == 0):
            if 1000 * abs(b - a) <= tol * a:
                return True
            return bool(flags & HALF_DOUBLE) and (1000 * abs(2 * b - a) <= tol * a or 1000 * abs(b - 2 * a) <= 2 * tol * a)
        return True

    out = []
    if seed_vec is None:
        if not 0 <= seed < n:
            return out
        out.append((seed, 0))
    else:
        cand = [(dist([int(x) for x in seed_vec], lib[j]), j) for j in range(n) if not masked(j)]
        if not cand:
            return out
        d, j = min(cand)
        out.append((j, d))
    for t in range(1, min(length, n)):
        p = out[t - 1][0]
        cand = []
        for j in range(n):
            if any(j == s for s, _ in out) or masked(j):
                continue
            if gap > 0 and tags[j] >= 0 and any(tags[out[u][0]] == tags[j] for u in range(max(0, t - gap), t)):
                continue
            if passes(p, j):
                cand.append((dist(lib[p], lib[j]), j))
        if not cand:
            break
        d, j = min(cand)
        out.append((j, d))
    return out


# ---------------------------------------------------------------------------
# attributes, rules and the named cases of the GPU tests

# tempos at both edges of each window of a previous song at 120.00 BPM with 50 per mille (w = 600, 2 w = 1200):
# equality on the boundary and one unit past it, for same, half and double time
EDGE_TEMPOS = (12000, 11400, 11399, 12600, 12601, 5700, 5699, 6300, 6301, 22800, 22799, 25200, 25201)


def random_attrs(n, seed, unknown=0.1, tempos=None):
    """keys uniform over 24 and tempos uniform over 60.00 .. 180.00 BPM (or drawn from `tempos`), a share `unknown` of
    each unknown: tempo 0, keys 24, 200 and 255"""
    rng = np.random.default_rng(seed)
    tempo = rng.integers(6000, 18001, size=n) if tempos is None else rng.choice(np.asarray(tempos), size=n)
    key = rng.integers(0, 24, size=n)
    tempo[rng.random(n) < unknown] = 0
    lost = rng.random(n) < unknown
    key[lost] = rng.choice([24, 200, 255], size=int(lost.sum()))
    return np.stack([tempo, key], axis=1).astype(np.int64)


def asymmetric_table(seed):
    """a third of all (a, b) allowed, the diagonal always, and no pair both ways but by chance; the ignored bits set"""
    rng = np.random.default_rng(seed)
    table = []
    for a in range(24):
        word = 1 << a | 0xA5000000
        for b in range(24):
            if rng.random() < 1 / 3:
                word |= 1 << b
        table.append(word)
    assert any((table[a] >> b & 1) != (table[b] >> a & 1) for a in range(24) for b in range(24))
    return table


def cases():
    """name -> keyword arguments of hmix()"""
    out = {}
    rng = np.random.default_rng(4321)
    # keys alone under an asymmetric table, unknown keys 24, 200 and 255 among them; more than two groups
    n = 257
    attrs = random_attrs(n, 1, unknown=0.12)
    attrs[[0, 1, 2], 1] = [24, 200, 255]
    rule = dict(key_ok=asymmetric_table(2), tempo_tol=0, flags=KEY)
    out["keys"] = dict(lib=R.random_lib(n, 11), attrs=attrs, rule=rule, seeds=np.arange(33, dtype=np.int32), length=12)
    # tempo alone at 50 per mille, the tempos from the edges of the windows of 120.00 BPM, some unknown
    n = 300
    attrs = random_attrs(n, 3, unknown=0.08, tempos=EDGE_TEMPOS + (12000,) * 5)
    attrs[:14, 0] = (12000,) + EDGE_TEMPOS
    rule = dict(key_ok=[0] * 24, tempo_tol=50, flags=TEMPO)
    out["tempo_edges"] = dict(lib=R.random_lib(n, 12), attrs=attrs, rule=rule,
                              seeds=rng.integers(0, n, size=20).astype(np.int32), length=10)
    # the same tempos with half and double time
    rule = dict(key_ok=[0] * 24, tempo_tol=50, flags=TEMPO | HALF_DOUBLE)
    seeds = rng.integers(0, n, size=18).astype(np.int32)
    seeds[:3] = [0, 5, 9]
    out["half_double"] = dict(lib=R.random_lib(n, 13), attrs=attrs, rule=rule, seeds=seeds, length=10)
    # everything at once: the wheel, tempo with half and double time, tags and a mask, an excluded seed
    n = 1025
    attrs = random_attrs(n, 4, unknown=0.1)
    tags = rng.integers(-1, 6, size=n).astype(np.int32)
    ex = rng.random(n) < 0.15
    seeds = rng.integers(0, n, size=17).astype(np.int32)
    ex[seeds[3]] = True
    out["wheel_rules"] = dict(lib=R.random_lib(n, 14), attrs=attrs, rule=camelot(150, KEY | TEMPO | HALF_DOUBLE),
                              seeds=seeds, length=12, tags=tags, gap=2, exclude=ex)
    # descriptor seeds: slot 0 under no pair rule, its pick's attribute binds slot 1; tags and a mask
    n = 400
    attrs = random_attrs(n, 5, unknown=0.1)
    lib = R.random_lib(n, 15)
    sd = R.random_lib(18, 16)
    sd[4] = lib[7]
    tags = rng.integers(0, 8, size=n).astype(np.int32)
    ex = rng.random(n) < 0.1
    ex[7] = False
    out["seed_desc"] = dict(lib=lib, attrs=attrs, rule=camelot(200, KEY | TEMPO), seed_desc=sd, length=10, tags=tags,
                            gap=3, exclude=ex)
    return out


# switch -> (case, row): the row of the case's output that the switch changes
SWITCH_CASE = {
    "table_transposed": ("keys", 0),
    "unknown_key_blocks": ("keys", 1),
    "key_ge_24_indexes_table": ("keys", 2),
    "unknown_tempo_blocks": ("tempo_edges", 0),
    "tol_of_candidate": ("tempo_edges", 1),
    "row_swap_attr": ("half_double", 0),
    "half_only": ("half_double", 2),
    "double_tol_not_doubled": ("half_double", 4),
    "rule_from_slot0": ("wheel_rules", 0),
    "seed_attr_ignored": ("wheel_rules", 3),   # the excluded seed: its attribute binds slot 1 all the same
    "blocked_lowers_bound": ("seed_desc", 0),
    "seed_desc_ruled": ("seed_desc", 4),
}
