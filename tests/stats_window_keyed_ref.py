"""Restatement, key patterns and plan builder of the statistics window by label (vst_cwct_stats_pool_keyed; test infrastructure
only; tests/test_stats_window_keyed_host.py and tests/test_gpu_stats_window_keyed.py).  Imports no GPU code.

pool_keyed_ref is include/vstnet.h ("Statistics window by label") in numpy: per slot r of the newest plan gather the record of
its label from every age (a miss: a record with n = 0, which the pool skips like any unusable age), then stats_window_ref.pool_ref
on the gathered block: dtype = float64 restates the device, dtype = longdouble is the truth.  Slots r >= n_slots of the newest plan
are dead: used = 0 and no record (the rows of `out` keep `fill`).
"""
import numpy as np

import stats_window_ref as R
from cwct_ops_ref import MAX_SLOTS, rec_len

PLAN_BYTES = 2344            # include/vstnet.h VST_LABEL_PLAN_BYTES
PLAN_LABELS = 8 + 2048 + 256  # {int n_slots, overflow; int hist_c[256], hist_s[256]; u8 lut[256]; u8 slot_label[32]}


def plan_bytes(labels, overflow=0, pad=0, stale=()):
    """A LabelPlan as the device lays it out, for the slot labels given (in slot order); slot_label beyond them = `pad` (the
    device writes 0), lut[label] = slot, 255 elsewhere.  The histograms are left at zero: the pool does not read them.
    stale: bytes that sit in slot_label right behind the live labels (what another tenant of the buffer left there): n_slots
    does not count them, so nothing may match them."""
    labels = [int(v) for v in labels]
    assert len(labels) <= MAX_SLOTS and len(set(labels)) == len(labels)
    raw = np.zeros(PLAN_BYTES, dtype=np.uint8)
    raw[:8].view(np.int32)[:] = (len(labels), overflow)
    lut = raw[8 + 2048:8 + 2048 + 256]
    lut[:] = 255
    for s, v in enumerate(labels):
        lut[v] = s
    raw[PLAN_LABELS:PLAN_LABELS + MAX_SLOTS] = pad
    raw[PLAN_LABELS:PLAN_LABELS + len(labels)] = labels
    stale = [int(v) for v in stale][:MAX_SLOTS - len(labels)]
    raw[PLAN_LABELS + len(labels):PLAN_LABELS + len(labels) + len(stale)] = stale
    return raw


def plan_labels(raw):
    """the slot labels of a LabelPlan's bytes, in slot order"""
    raw = np.asarray(raw, dtype=np.uint8)
    n = int(raw[:4].view(np.int32)[0])
    return [int(v) for v in raw[PLAN_LABELS:PLAN_LABELS + n]]


def gather(records, labels):
    """records[a]: [max_slots, rec], labels[a]: the slot labels of age a -> (blocks [n0, rec] per age, in age 0's slot order; hit
    [ages, n0] bool).  A miss is a zero record (n = 0)."""
    n0, length = len(labels[0]), np.asarray(records[0]).shape[-1]
    blocks, hit = [], np.zeros((len(records), n0), dtype=bool)
    for a, (rec, lab) in enumerate(zip(records, labels)):
        blk = np.zeros((n0, length), dtype=np.float64)
        for r, key in enumerate(labels[0]):
            if key in lab:
                blk[r] = np.asarray(rec, dtype=np.float64)[lab.index(key)]
                hit[a, r] = True
        blocks.append(blk)
    return blocks, hit


MUTANTS = {
    "unbounded_search": "the key lookup of an older age runs over all of slot_label, past the age's n_slots (the zero padding "
                        "and whatever is stale there match; the first match wins)",
}


def pool_keyed_ref(records, labels, weights, cut, dtype=np.float64, fill=np.nan, plans=None, mut=()):
    """-> (out [max_slots, rec] in `dtype`, rows >= len(labels[0]) = fill; used int32 [max_slots]).  mut (with `plans`, the
    ages' LabelPlan bytes): a switch of MUTANTS makes the lookup wrong in one way."""
    max_slots, length = np.asarray(records[0]).shape
    if "unbounded_search" in mut:
        labels = [labels[0]] + [[int(v) for v in np.asarray(p)[PLAN_LABELS:PLAN_LABELS + max_slots]] for p in plans[1:]]
    out = np.full((max_slots, length), fill, dtype=dtype)
    used = np.zeros(max_slots, dtype=np.int32)
    n0 = len(labels[0])
    if n0:
        blocks, _ = gather(records, labels)
        out[:n0], used[:n0] = R.pool_ref(blocks, weights, cut, dtype)
    return out, used


# ============================================================================================================ the key patterns
# name -> f(max_slots, ages) -> the slot labels per age (age 0 first).  Labels are drawn from 0..255 in increasing order (as the
# device plans them) unless the pattern is about the order.
def _base(max_slots):
    return [3 + 7 * s for s in range(max_slots)]            # (label 0 is not among them: the padding cannot match by accident)


def _identity(ms, ages):
    return [_base(ms) for _ in range(ages)]


def _reversed_older(ms, ages):
    return [_base(ms)] + [_base(ms)[::-1] if a % 2 else _base(ms)[1:] + _base(ms)[:1] for a in range(1, ages)]


def _missing_middle(ms, ages):
    lab = _identity(ms, ages)
    lab[1] = [v for v in lab[1] if v != _base(ms)[1]]       # label of slot 1 is not in age 1: the later slots move down by one
    return lab


def _missing_everywhere(ms, ages):
    return [_base(ms)] + [[v for v in _base(ms) if v != _base(ms)[0]] for _ in range(1, ages)]


def _empty_older(ms, ages):
    """label 0 is live in every age but the oldest, which has n_slots = 0 (its slot_label bytes are stale: stale_labels below)"""
    new = [0] + _base(ms)[:ms - 1]
    return [list(new) for _ in range(ages - 1)] + [[]]


def _short_newest(ms, ages):
    return [_base(ms)[:max(1, ms // 2 - 1)]] + [_base(ms) for _ in range(1, ages)]


def _label_zero(ms, ages):
    """label 0 is live in age 0; age 1 holds fewer than 32 slots and not label 0: its zero padding must not match"""
    new = [0] + _base(ms)[:ms - 1]
    return [new, _base(ms)[:ms - 1][:min(ms - 1, 5)]] + [new for _ in range(2, ages)]


def stale_labels(pattern, ms, labels):
    """per age the bytes behind the live labels in slot_label: nothing (the device's zero padding), except in the n_slots = 0
    age of "empty_older", which still holds the labels of age 0 - label 0 among them - from an earlier tenant"""
    return [list(labels[0]) if pattern == "empty_older" and not lab else [] for lab in labels]


def keyed_plans(pattern, ms, labels):
    """the LabelPlan bytes of every age of a keyed_input"""
    return [plan_bytes(lab, stale=st) for lab, st in zip(labels, stale_labels(pattern, ms, labels))]


KEY_PATTERNS = {
    "identity": _identity,
    "reversed_older": _reversed_older,
    "missing_middle": _missing_middle,
    "missing_everywhere": _missing_everywhere,
    "empty_older": _empty_older,
    "short_newest": _short_newest,
    "label_zero": _label_zero,
}


def keyed_input(N, max_slots, pattern, ages=3, cut_label=False, seed=0):
    """-> (records: `ages` arrays [max_slots, rec] newest first; labels per age; weights; cut).
    Every label has one underlying distribution, so the record of a label is comparable across ages wherever it sits.
    Rows past an age's slots: NaN in age 0 (a dead slot is never read); in every older age a DECOY, a valid record (n >= 2) of
    another distribution - what the frame that held the ring slot before left there.  A lookup that ran past n_slots (into the
    zero padding: label 0; into stale labels) would find one, pool it and change `used` and the record.
    cut_label: the label of age 0's slot 0 is another scene in age 1 (by its mean: far over 4 x CUT), every other label is not."""
    rng = np.random.default_rng(1000 * N + 10 * max_slots + seed + sum(map(ord, pattern)))
    labels = KEY_PATTERNS[pattern](max_slots, ages)
    scales = {v: (rng.permutation(np.logspace(-2, 2, N)) if N > 1 else np.array([3.0])) for v in range(256)}
    means = {v: rng.uniform(-100.0, 100.0, N) * scales[v] for v in range(256)}
    records = []
    for a, lab in enumerate(labels):
        blk = np.full((max_slots, rec_len(N)), np.nan)
        for s, v in enumerate(lab):
            L = 600 + 31 * a + 3 * s
            mu = means[v] + 0.1 * scales[v] * rng.standard_normal(N)
            if cut_label and a == 1 and v == labels[0][0]:
                mu = mu + 20.0 * scales[v]
            x = (mu[:, None] + scales[v][:, None] * rng.standard_normal((N, L))).astype(np.float32)
            blk[s] = R.stats64(x)
        for s in range(len(lab), max_slots if a else 0):
            v = 255 - s                                      # (no pattern uses labels this high)
            x = (5.0 * scales[v][:, None] * (1.0 + rng.standard_normal((N, 400 + s)))).astype(np.float32)
            blk[s] = R.stats64(x)
        records.append(blk)
    weights = np.array([0.5 ** a for a in range(ages)])
    return records, labels, weights, (R.CUT if cut_label else 0.0)


# ==================================================================================================== the ring, with plan copies
def replay_ring(window, depth, start, frames=50):
    """FramePipeline.run's schedule under stats_by_label, restated (tests/test_stats_window_host.py has the unkeyed one): every
    ring slot holds a (record, plan copy) pair written by one frame; frame t writes slot t % R and its pool reads the pairs of
    frames t - 1 .. t - window + 1.  The frame's OWN plan buffer is its frame ring slot t % depth, rewritten by frame t + depth.
    Returns (slot reuse was always safe, the pairs read were always the right frames', some read would have been wrong had the
    pool read the frames' own plan buffers)."""
    slots = window + depth
    first = max(0, start - (window - 1))
    rec_of, plan_of, reader, retired = [None] * slots, [None] * slots, [None] * slots, None
    own_plan = [None] * max(depth, 1)
    safe = right = True
    own_would_fail = False
    for t in range(first, start + frames):
        j = t % slots
        safe &= reader[j] is None or (retired is not None and reader[j] <= retired)
        rec_of[j], plan_of[j], reader[j] = t, t, None
        own_plan[t % max(depth, 1)] = t
        for age in range(1, min(window, t - first + 1)):
            k = (t - age) % slots
            right &= rec_of[k] == t - age and plan_of[k] == t - age
            own_would_fail |= own_plan[(t - age) % max(depth, 1)] != t - age
            if t >= start:
                reader[k] = t
        if t >= start and t - start + 1 > depth - 1:
            retired = t - (depth - 1)
    return safe, right, own_would_fail
