"""--stats_by_label on the host: the keyed restatement against fp64 statistics of the per-label union of the frames' pixels, the
script's argument table, the warm-up counts of the two windows together, the record ring's schedule with the plan copies, and the
new entry point in the header and the built library."""
import os
import re
import subprocess

import numpy as np
import pytest

import stats_window_keyed_ref as K
import stats_window_ref as R
from cwct_ops_ref import stats64, stats_err

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restatement_against_the_union_of_each_labels_pixels():
    """Three frames whose label sets differ and whose slot orders are permuted; equal weights, no cut: every live label's pooled
    record is the record of the concatenated pixels of that label over the frames that hold it."""
    rng = np.random.default_rng(5)
    for N in (1, 7, 32):
        scales = np.logspace(-2, 2, N) if N > 1 else np.array([2.0])
        labels = [[4, 0, 9, 200], [9, 4, 17], [200, 9, 0, 4, 33]]            # newest first; label 0 among the keys
        pixels = [{v: ((rng.uniform(-100, 100, N) * scales)[:, None] + scales[:, None]
                       * rng.standard_normal((N, 200 + 37 * a + 5 * s))).astype(np.float32) for s, v in enumerate(lab)}
                  for a, lab in enumerate(labels)]
        records = []
        for lab, px in zip(labels, pixels):
            blk = np.full((8, R.rec_len(N)), np.nan)
            for s, v in enumerate(lab):
                blk[s] = stats64(px[v])
            records.append(blk)
        got, used = K.pool_keyed_ref(records, labels, np.ones(3), 0.0)
        assert used.tolist() == [3, 2, 3, 2, 0, 0, 0, 0] and np.isnan(got[4:]).all()
        for r, v in enumerate(labels[0]):
            want = stats64(np.concatenate([px[v] for px in pixels if v in px], axis=1))
            ec, em = stats_err(got[r], want, N)
            print(f"keyed union N={N} label {v}: frames {used[r]} cov {ec:.2e} mean {em:.2e}")
            assert got[r, 0] == want[0]
            assert ec <= 2.0 ** -40 and em <= 2.0 ** -40


def test_key_patterns_are_what_they_are_named():
    for ms in (8, 32):
        for name, make in K.KEY_PATTERNS.items():
            lab = make(ms, 3)
            assert len(lab) == 3 and all(len(set(x)) == len(x) <= ms for x in lab), name
        assert len(K.KEY_PATTERNS["short_newest"](ms, 3)[0]) < ms
        z = K.KEY_PATTERNS["label_zero"](ms, 3)
        assert z[0][0] == 0 and 0 not in z[1] and len(z[1]) < 32
        assert K.KEY_PATTERNS["empty_older"](ms, 3)[2] == []
        m = K.KEY_PATTERNS["missing_middle"](ms, 3)
        assert m[0][1] not in m[1] and m[0][1] in m[2]
        e = K.KEY_PATTERNS["missing_everywhere"](ms, 3)
        assert all(e[0][0] not in x for x in e[1:])
    # the two bounds of the key lookup: behind the live slots of an older age sit valid records and (label_zero) the zero padding
    # or (empty_older: n_slots = 0) stale labels, label 0 among them; a lookup that ran past n_slots pools them
    for ms in (8, 32):
        for name in ("label_zero", "empty_older"):
            records, labels, w, cut = K.keyed_input(7, ms, name)
            plans = K.keyed_plans(name, ms, labels)
            n0 = len(labels[0])
            assert labels[0][0] == 0 and [K.plan_labels(p) for p in plans] == labels
            for a in range(1, 3):
                assert (records[a][len(labels[a]):, 0] >= 2).all() and np.isfinite(records[a]).all()
            got, used = K.pool_keyed_ref(records, labels, w, cut)
            bad, loose = K.pool_keyed_ref(records, labels, w, cut, plans=plans, mut=("unbounded_search",))
            if name == "label_zero":
                assert used[0] == 2 and loose[0] == 3 and not (plans[1][K.PLAN_LABELS + len(labels[1]):K.PLAN_LABELS + 32]).any()
            else:
                assert set(used[:n0]) == {2} and set(loose[:n0]) == {3}
                assert list(plans[2][K.PLAN_LABELS:K.PLAN_LABELS + n0]) == labels[0]
            assert not np.array_equal(got[0].view(np.uint64), bad[0].view(np.uint64))
    records, labels, w, cut = K.keyed_input(7, 8, "identity", cut_label=True)
    trace = []
    blocks, _ = K.gather(records, labels)
    _, used = R.pool_ref(blocks, w, cut, np.longdouble, trace=trace)
    assert used.tolist() == [1] + [3] * 7                                    # the cut is on one label only
    for r, a, d, limit in trace:
        assert d < limit / 4 or d > 4 * limit, (r, a, float(d / limit))
    raw = K.plan_bytes([5, 0, 9])
    assert raw.size == K.PLAN_BYTES and K.plan_labels(raw) == [5, 0, 9]


def test_script_argument_table(capsys):
    import video_transfer as vt
    parser = vt.build_parser()
    base = ["--video", "clip", "--style", "s.png"]
    maps = ["--content_seg_dir", "maps", "--style_seg", "s_seg.png"]
    auto = ["--auto_seg", "--synthetic_seg_weights", "--no_seg_remap"]

    def check(argv):
        args = parser.parse_args(base + argv)
        vt.check_seg_args(parser, args)
        vt.check_window_args(parser, args)
        vt.check_stats_args(parser, args)
        return args

    def fails(argv, text):
        with pytest.raises(SystemExit) as e:
            check(argv)
        err = capsys.readouterr().err
        assert e.value.code == 2 and text in err, err
    assert not check([]).stats_by_label
    a = check(["--stats_window", "3", "--stats_by_label"] + maps)                 # the flag lifts the two refusals
    assert a.stats_by_label and a.stats_window == 3
    a = check(["--stats_window", "3", "--stats_by_label", "--seg_window", "2", "--stats_cut", "0.01"] + auto)
    assert a.stats_by_label and a.seg_window == 2
    fails(["--stats_window", "3"] + maps, "not with --content_seg_dir or --auto_seg")      # without it the old text stays
    fails(["--stats_window", "3"] + auto, "not with --content_seg_dir or --auto_seg")
    fails(["--stats_window", "3"] + maps, "--stats_by_label")                              # ... with a hint
    fails(["--stats_by_label"], "--stats_window W with W > 1")
    fails(["--stats_by_label"] + maps, "--stats_window W with W > 1")
    fails(["--stats_window", "3", "--stats_by_label"], "--content_seg_dir or --auto_seg")
    fails(["--stats_window", "3", "--stats_by_label", "--content_seg", "c.png", "--style_seg", "s_seg.png"],
          "--content_seg_dir or --auto_seg")
    fails(["--stats_window", "3", "--stats_by_label", "--map_drift"] + maps, "--map_drift")


def test_warmup_counts():
    """(logit-only, statistics) warm-up frames over a small grid, against the definition: frame f's window holds the records of
    the Wt - 1 frames before it; the oldest of those is labelled from the logits of the Ws - 1 frames before IT."""
    from video_transfer import warmup_frames
    from vstnet_amd.pipeline import warmup_counts
    for ws in (1, 2, 3, 8):
        for wt in (1, 2, 4, 8):
            for first in (0, 1, 2, 3, 5, 9, 20):
                stats = [f for f in range(first - (wt - 1), first) if f >= 0]
                oldest = stats[0] if stats else first
                logits = [f for f in range(oldest - (ws - 1), oldest) if f >= 0]
                assert warmup_counts(ws, wt, first) == (len(logits), len(stats)), (ws, wt, first)
                assert warmup_frames(first, ws, wt) == tuple(logits + stats), (ws, wt, first)
    assert warmup_counts(3, 4, 2) == (0, 2) and warmup_counts(3, 4, 4) == (1, 3) and warmup_counts(3, 4, 100) == (2, 3)
    assert warmup_frames(4, 3, 1) == (2, 3) and warmup_frames(4, 1, 3) == (2, 3) and warmup_frames(0, 8, 8) == ()


@pytest.mark.parametrize("window", range(1, 9))
def test_ring_schedule_with_plan_copies(window):
    from vstnet_amd.pipeline import logit_ring_slots
    seen_own_fail = False
    for depth in range(1, 7):
        assert logit_ring_slots(window, depth) == window + depth
        for start in (0, 5):
            safe, right, own_fail = K.replay_ring(window, depth, start)
            assert safe and right, (window, depth, start)
            assert own_fail == (window - 1 >= depth), (window, depth, start)       # why the ring keeps copies of the plans
            seen_own_fail |= own_fail
    assert seen_own_fail == (window >= 2)


@pytest.fixture(scope="module")
def lib():
    from vstnet_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_library_exports_the_keyed_entry(lib):
    import inspect
    from vstnet_amd import _lib
    from vstnet_amd.cwct import cWCT
    from vstnet_amd.pipeline import FramePipeline
    hdr = open(os.path.join(REPO, "include", "vstnet.h")).read()
    assert re.search(r"\bint\s+vst_cwct_stats_pool_keyed\s*\(", hdr) and "vst_cwct_stats_pool_keyed" in _lib.EXPORTS
    assert "Statistics window by label (version 114" in hdr
    assert hasattr(lib, "vst_cwct_stats_pool_keyed") and lib.vst_version() >= 114
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT vst_cwct_stats_pool_keyed\b", out)
    m = re.search(r"#define\s+VST_LABEL_PLAN_BYTES\s+(\d+)", hdr)
    assert m and int(m.group(1)) == _lib.LABEL_PLAN_BYTES == K.PLAN_BYTES
    assert "plans" in inspect.signature(cWCT.pool_stats).parameters
    assert "by_label" in inspect.signature(cWCT.frame_stats).parameters
    assert "by_label" in inspect.signature(cWCT.transfer_with_plan).parameters
    assert "stats_by_label" in inspect.signature(FramePipeline.__init__).parameters
    assert "warmup_masks" in inspect.signature(FramePipeline.run).parameters
    table = open(_lib.RESOURCES_PATH).read() if os.path.exists(_lib.RESOURCES_PATH) else ""
    for line in table.splitlines():                          # (the table is written by a build; a prebuilt library has none)
        if "cwct_stats_pool_keyed_kernel" in line and "ScratchSize" in line:
            assert line.rstrip().endswith(": 0"), line


def test_keyed_argument_errors_come_before_any_launch(lib):
    """No GPU here: every one of these returns before it touches the device.  The unkeyed entry's table, with a plan per age
    (never dereferenced), then the plan pointers' own."""
    import ctypes as C
    vp = C.c_void_p
    plans = (vp * 2)(0x8000000, 0x8001000)
    for name, status, a in R.pool_error_cases():
        assert lib.vst_cwct_stats_pool_keyed(a[0], plans, *a[1:], None) == status, name
    good = next(a for name, _, a in R.pool_error_cases() if name == "cut negative")
    good = good[:5] + (0.0,) + good[6:]
    assert lib.vst_cwct_stats_pool_keyed(good[0], None, *good[1:], None) == -1
    assert lib.vst_cwct_stats_pool_keyed(good[0], (vp * 2)(0x8000000, 0), *good[1:], None) == -1
    assert lib.vst_cwct_stats_pool_keyed(good[0], (vp * 2)(0x8000000, 0x8001002), *good[1:], None) == -1
