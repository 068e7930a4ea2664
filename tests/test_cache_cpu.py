"""The transposition cache's pure parts (csrc/az_cache.h), on the CPU: the
state word, the bucket of a hash, the candidate scan of a lookup, the victim
choice of an insert and the generation size.  tests/native/cache_check.cpp is
the host program and only prints what the header returns; the inputs are
drawn here and the expectations computed here, in plain Python, from the
protocol's description (not from the header's loops).  The lock-free parts
(lookup, claim, publish) are checked on the device by the self-play tests
against the oracle.
"""
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(REPO, "tests", "native")
EXE = os.path.join(NATIVE, "_build", "cache_check")

EMPTY, CLAIMED, READY = 0, 1, 2
BUCKET = 16
GEN_MASK = 0x3FFF  # the generation field wraps at 2^14
EVICT_AGE = 2
M32 = 0xFFFFFFFF


@pytest.fixture(scope="module")
def exe():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17",
                    os.path.join(NATIVE, "cache_check.cpp"), "-o", EXE], check=True, timeout=600)
    return EXE


def _run(exe, tmp_path, cmd, records, dtype):
    """one output line (split into ints) per record"""
    path = tmp_path / f"{cmd}.bin"
    np.asarray(records, dtype=dtype).tofile(path)
    lines = subprocess.run([exe, cmd, str(path)], capture_output=True, text=True, check=True,
                           timeout=60).stdout.splitlines()
    assert len(lines) == len(records)
    return [[int(v) for v in line.split()] for line in lines]


def word(fp, gen, status):
    return (fp << 16) | ((gen & GEN_MASK) << 2) | status


def age(w, now):
    return (now - (w >> 2)) & GEN_MASK


# ---------------------------------------------------------------- state word
def test_state_word_round_trip_and_age(exe, tmp_path):
    rng = np.random.RandomState(1)
    recs = []
    for g in [0, 0x3FFE, 0x3FFF, 0x4000, 2 ** 32 - 1]:
        for k in range(4):
            for status in (EMPTY, CLAIMED, READY):
                recs.append([int(rng.randint(0, 1 << 16)), g, status, (g + k) & M32])
    recs.append([0xFFFF, GEN_MASK, READY, GEN_MASK])  # every field full
    out = _run(exe, tmp_path, "word", recs, np.uint32)
    for (fp, g, status, now), (w, a) in zip(recs, out):
        assert w >> 16 == fp and w & 3 == status and (w >> 2) & GEN_MASK == g & GEN_MASK, (fp, g, status)
        assert a == (now - g) & GEN_MASK, (g, now)
    # the issue's statement itself: age k, k generations after a Ready word's stamp
    ready = [(r, o) for r, o in zip(recs, out) if r[2] == READY][:20]
    assert [o[1] for _, o in ready] == [0, 1, 2, 3] * 5


def test_fingerprint_is_hash_bits_48_to_63(exe, tmp_path):
    rng = np.random.RandomState(2)
    hs = [int(x) for x in rng.randint(0, 1 << 32, 64).astype(np.uint64) << np.uint64(32) |
          rng.randint(0, 1 << 32, 64).astype(np.uint64)]
    hs += [0, 1 << 48, (1 << 48) - 1, (1 << 64) - 1, 0xABCD << 48]
    out = _run(exe, tmp_path, "fp", hs, np.uint64)
    assert [o[0] for o in out] == [h >> 48 for h in hs]
    assert out[-1][0] == 0xABCD and out[-3][0] == 0


# -------------------------------------------------------------- cache_bucket
def test_bucket_of_a_hash(exe, tmp_path):
    rng = np.random.RandomState(3)
    recs, triples = [], []
    for log2 in [4, 5, 6, 10, 16, 26, 28, 30]:
        mask = (1 << log2) - 1
        for _ in range(40):
            lo, hi = int(rng.randint(0, 1 << 32)), int(rng.randint(0, 1 << 32))
            triples.append(len(recs))
            recs.append([(hi << 32) | lo, mask])
            recs.append([lo, mask])                          # the same low word, other high bits
            recs.append([((hi ^ M32) << 32) | lo, mask])
        recs.append([(1 << 64) - 1, mask])
    out = [o[0] for o in _run(exe, tmp_path, "bucket", recs, np.uint64)]
    for (h, mask), b in zip(recs, out):
        assert b % BUCKET == 0 and b <= mask - 15, (h, mask, b)
        assert b == (h & M32) & mask & ~15, (h, mask, b)
        if mask == 15:
            assert b == 0
    for i in triples:
        assert out[i] == out[i + 1] == out[i + 2]  # only the low 32 bits count


# ------------------------------------------------------------ random buckets
def random_bucket(rng, fps, gen):
    """a non-empty prefix of 0..16 slots (ages 0..5 behind `gen`, in some buckets all
    below the eviction age), empty after it; sometimes a stray non-empty word past
    the first empty slot"""
    n = int(rng.randint(0, BUCKET + 1))
    ages = 6 if rng.rand() < 0.7 else EVICT_AGE
    w = [0] * BUCKET
    for k in range(n):
        status = READY if rng.rand() < 0.8 else CLAIMED
        w[k] = word(int(fps[rng.randint(len(fps))]), gen - int(rng.randint(0, ages)), status)
    if n < BUCKET - 1 and rng.rand() < 0.3:
        k = int(rng.randint(n + 1, BUCKET))
        w[k] = word(int(fps[rng.randint(len(fps))]), gen - int(rng.randint(0, 6)), READY)
    return w


def random_gen(rng):
    """a generation counter, sometimes just past a wrap of the 2^14 field"""
    r = rng.rand()
    if r < 0.4:
        return (int(rng.randint(1, 8)) << 14) + int(rng.randint(0, 5))
    if r < 0.5:
        return int(rng.randint(0, 5))  # the first generations after a clear (ages wrap below 0)
    return int(rng.randint(0, 1 << 20))


# ------------------------------------------------------------ candidate scan
def expected_candidates(w, fp):
    live = w[:w.index(EMPTY)] if EMPTY in w else w  # nothing past the first empty slot
    return sum(1 << k for k, st in enumerate(live) if st & 3 == READY and st >> 16 == fp)


def test_candidate_scan(exe, tmp_path):
    rng = np.random.RandomState(4)
    fps = [0x1234, 0x1235, 0xFFFF, 0x0000, 0x8000]  # few: matches are common
    recs = []
    for _ in range(2000):
        recs.append(random_bucket(rng, fps, random_gen(rng)) + [int(fps[rng.randint(len(fps))])])
    F, G = 0x1234, 0x1235
    full = [word(F if k % 5 == 0 else G, 7, READY) for k in range(BUCKET)]
    hand = {
        "an empty word hides the match after it": ([word(G, 1, READY), 0, word(F, 1, READY)] + [0] * 13, F, 0),
        "claimed with the fingerprint": ([word(F, 1, CLAIMED), word(F, 1, READY)] + [0] * 14, F, 0b10),
        "ready with another fingerprint": ([word(G, 1, READY), word(F, 1, READY)] + [0] * 14, G, 0b01),
        "several matches, in slot order": ([word(F, 1, READY), word(G, 2, READY), word(F, 3, READY),
                                            word(F, 0x3FFF, READY)] + [0] * 12, F, 0b1101),
        "a full bucket": (full, F, 0b1000010000100001),
        "a full bucket without a match": (full, 0x4321, 0),
        "an empty bucket": ([0] * BUCKET, 0, 0),
        "fingerprint 0 in a ready word": ([word(0, 3, READY)] + [0] * 15, 0, 1),
    }
    for w, fp, want in hand.values():
        assert expected_candidates(w, fp) == want  # the expectation itself, on cases worked by hand
        recs.append(list(w) + [fp])
    out = [o[0] for o in _run(exe, tmp_path, "scan", recs, np.uint32)]
    want = [expected_candidates(r[:BUCKET], r[BUCKET]) for r in recs]
    assert out == want
    assert sum(bin(m).count("1") > 1 for m in want) > 50 and want.count(0) > 50  # both kinds occur


# -------------------------------------------------------------- victim choice
def expected_victim(w, gen, tried, evict):
    """(slot, the word expected there, empty?): the first empty slot not tried; else,
    with eviction on, the oldest entry of age >= 2 not tried, the first of equal ages
    (whatever its status bits: the rule as it stands); else none"""
    free = [k for k in range(BUCKET) if not (tried >> k) & 1]
    empties = [k for k in free if w[k] == EMPTY]
    if empties:
        return empties[0], 0, 1
    old = [k for k in free if age(w[k], gen) >= EVICT_AGE] if evict else []
    if not old:
        return -1, 0, 0
    k = min(old, key=lambda k: (-age(w[k], gen), k))
    return k, w[k], 0


def test_victim_choice(exe, tmp_path):
    rng = np.random.RandomState(5)
    fps = [0x1234, 0xFFFF, 0x0001]
    recs = []
    for i in range(3000):
        gen = random_gen(rng)
        w = random_bucket(rng, fps, gen)
        tried = int(rng.randint(0, 1 << 16)) if rng.rand() < 0.7 else 0
        if rng.rand() < 0.3:  # every empty slot lost already: the eviction rule decides
            tried |= sum(1 << k for k in range(BUCKET) if w[k] == EMPTY)
        recs.append(w + [gen & M32, tried, (i % 2) * int(rng.randint(1, 1 << 20))])  # gen_size: 0 = eviction off
    F = 0x1234
    g = (3 << 14) + 1  # just past a wrap: ages count through it
    full = lambda ages: [word(F, g - a, READY) for a in ages]  # noqa: E731
    hand = {
        "an empty slot beats an older entry before it": (full([5, 4]) + [0] * 14, g, 0, 1, (2, 0, 1)),
        "the first of equal ages": (full([1, 3, 0, 3, 2, 3] + [0] * 10), g, 0, 1, (1, word(F, g - 3, READY), 0)),
        "the oldest, not the first old one": (full([2, 3, 5, 4] + [1] * 12), g, 0, 1, (2, word(F, g - 5, READY), 0)),
        "age 1 is never taken": (full([1] * 16), g, 0, 1, (-1, 0, 0)),
        "age 0 and 1 only": (full([0, 1] * 8), g, 0, 1, (-1, 0, 0)),
        "a tried empty slot is skipped": (full([0]) + [0] * 15, g, 0b10, 1, (2, 0, 1)),
        "a tried old entry is skipped": (full([5, 4, 3] + [0] * 13), g, 0b001, 1, (1, word(F, g - 4, READY), 0)),
        "every slot tried": (full([5] * 16), g, 0xFFFF, 1, (-1, 0, 0)),
        "eviction off: old entries stay": (full([5] * 16), g, 0, 0, (-1, 0, 0)),
        "eviction off: an empty slot is taken": (full([5] * 15) + [0], g, 0, 0, (15, 0, 1)),
        "eviction off: every empty slot tried": (full([5] * 14) + [0, 0], g, 0xC000, 0, (-1, 0, 0)),
        "an empty bucket": ([0] * 16, 0, 0, 0, (0, 0, 1)),
    }
    for w, gen, tried, evict, want in hand.values():
        assert expected_victim(w, gen, tried, evict) == want  # the expectation itself, on cases worked by hand
        recs.append(list(w) + [gen & M32, tried, evict])
    out = [tuple(o) for o in _run(exe, tmp_path, "victim", recs, np.uint32)]
    want = [expected_victim(r[:BUCKET], r[BUCKET], r[BUCKET + 1], r[BUCKET + 2] != 0) for r in recs]
    assert out == want
    n = 3000  # the random part: each outcome occurs, with eviction off (no entry evicted then) and on
    for evict in (0, 1):
        part = [w for r, w in zip(recs[:n], want[:n]) if (r[BUCKET + 2] != 0) == bool(evict)]
        took_empty = sum(w[2] == 1 for w in part)
        evicted = sum(w[0] >= 0 and w[2] == 0 for w in part)
        nothing = sum(w[0] < 0 for w in part)
        assert took_empty > 100 and nothing > 100, (evict, took_empty, evicted, nothing)
        assert (evicted > 100) if evict else (evicted == 0), (evict, evicted)


# ------------------------------------------------------------ cache_gen_size
def test_gen_size(exe, tmp_path):
    window = 3 * 32 * 50  # three moves of 32 slots x 50 simulations (the Connect-N engine's argument)
    recs = [[1 << 17, window], [1 << 16, window], [1 << 14, window], [1 << 6, 0], [1 << 4, 0]]
    out = [o[0] for o in _run(exe, tmp_path, "gen_size", recs, np.uint64)]
    assert out == [8192, 4801, 0, 4, 1]
    # the rule: max(cap / 16, window + 1), or 0 (no eviction) when that is more than cap / 4
    more = [[1 << k, w] for k in (4, 8, 20, 26, 28, 30) for w in (0, 1, 15, 16, (1 << k) // 4 - 1, (1 << k) // 4)]
    got = [o[0] for o in _run(exe, tmp_path, "gen_size", more, np.uint64)]
    for (cap, w), g in zip(more, got):
        want = max(cap // 16, w + 1)
        assert g == (want if want <= cap // 4 else 0), (cap, w, g)
