"""--stats_window on the host: the union identity of the pooled record, the mutants of the reference against the GPU test's
bound, the record ring's size against a simulation of the frame loop's schedule (with warm-up), the parser, the new entry
point in the header and the built library with its argument errors, and the margin the cut tests rely on."""
import os
import re
import subprocess

import numpy as np
import pytest

import stats_window_ref as R
from cwct_ops_ref import stats64, stats_err

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("frames", (2, 3, 8))
def test_union_identity(frames):
    """Equal weights, no cut: the pooled record is the record of the concatenated pixels (what the reference's whitening
    computes on them, models/cWCT.py:134-149)."""
    rng = np.random.default_rng(frames)
    for N in (1, 7, 32):
        scales = np.logspace(-2, 2, N) if N > 1 else np.array([2.0])
        xs = [((rng.uniform(-100, 100, N) * scales)[:, None] + scales[:, None] * rng.standard_normal((N, 300 + 41 * a)))
              .astype(np.float32) for a in range(frames)]
        got, used = R.pool_ref([stats64(x) for x in xs], np.ones(frames), 0.0)
        want = stats64(np.concatenate(xs, axis=1))
        ec, em = stats_err(got[0], want, N)
        print(f"union identity W={frames} N={N}: cov {ec:.2e} mean {em:.2e}")
        assert used[0] == frames and got[0, 0] == want[0]
        assert ec <= 2.0 ** -40 and em <= 2.0 ** -40


def test_case_table():
    """The table reaches every value of every axis, its constructions give the `used` they are meant to, and every cut decision
    in it has a margin of 4 to either side of the threshold: no rounding decides one."""
    assert {c[0] for c in R.CASES} == set(R.WIDTHS) and {c[1] for c in R.CASES} == {1, 8, 32}
    assert all(c[1] < 32 or c[0] <= 32 for c in R.CASES)
    assert {c[2] for c in R.CASES} == {1, 2, 3, 8} and {1.0, 0.5} <= {c[3] for c in R.CASES}
    assert {c[4] for c in R.CASES} == {"none", "age0", "middle", "all_but_0"} and {c[5] for c in R.CASES} == {False, True}
    assert {c[6] for c in R.CASES} == {"none", "age1", "age3", "age2_behind_unusable"}
    assert len({R.case_id(c) for c in R.CASES}) == len(R.CASES)
    counts = set()
    for case in R.CASES:
        if case[0] > 32:
            continue
        records, weights, cut = R.case_input(case)
        trace = []
        _, used = R.pool_ref(records, weights, cut, np.longdouble, trace=trace)
        assert np.array_equal(used, R.expected_used(case)), R.case_id(case)
        assert np.array_equal(R.pool_ref(records, weights, cut)[1], used)
        for r, a, d, limit in trace:
            assert d < limit / 4 or d > 4 * limit, (R.case_id(case), r, a, float(d / limit))
        counts |= {float(rec[r, 0]) for rec in records for r in range(case[1])}
    assert {0.0, 1.0} <= counts and min(counts) < 0           # n = 0, n = 1 and a prefactored record are all in there


def test_mutants_exceed_the_bound():
    """Every mutant of the reference is further than 1.25 x FACTOR x max(e64, 2^-53) from the truth at one case at least."""
    worst = {m: (0.0, None) for m in R.MUTANTS}
    for case in R.CASES:
        if case[0] > 32:
            continue
        records, weights, cut = R.case_input(case)
        truth, used = R.pool_ref(records, weights, cut, np.longdouble)
        r64, _ = R.pool_ref(records, weights, cut)
        assert R.pool_ratio(r64, r64, truth, used, case[0])[0] <= 1.0
        for m in R.MUTANTS:
            if worst[m][0] == np.inf:
                continue
            got, _ = R.pool_ref(records, weights, cut, mut=(m,))
            ratio = R.pool_ratio(got, r64, truth, used, case[0])[0]
            if ratio > worst[m][0]:
                worst[m] = (ratio, R.case_id(case))
    for m, (ratio, cid) in worst.items():
        print(f"mutant {m}: ratio {ratio:.3g} at {cid}")
        assert ratio > 1.25 * R.FACTOR, m


@pytest.mark.parametrize("window", range(1, 9))
def test_ring_size_and_slot_reuse(window):
    """FramePipeline.run's schedule, restated with warm-up frames: the up to window - 1 warm-up frames write their slots and
    are never retired (the host waits for them when their frame ring slot is filled again, so they count as complete from then
    on); frame t is submitted, then - once depth - 1 newer frames are queued - frame t - (depth - 1) is retired.  Frame t
    writes slot t % R and reads the slots of frames t - 1 .. t - window + 1."""
    from vstnet_amd.pipeline import logit_ring_slots
    for depth in range(1, 7):
        slots = logit_ring_slots(window, depth)
        assert slots == window + depth
        for start in (0, 5):
            first = max(0, start - (window - 1))
            holds, reader, retired = [None] * slots, [None] * slots, None
            for t in range(first, start + 50):
                j = t % slots
                assert reader[j] is None or (retired is not None and reader[j] <= retired), (window, depth, t)
                holds[j], reader[j] = t, None
                for age in range(1, min(window, t - first + 1)):
                    k = (t - age) % slots
                    assert holds[k] == t - age, (window, depth, t, age)
                    if t >= start:
                        reader[k] = t
                if t >= start and t - start + 1 > depth - 1:
                    retired = t - (depth - 1)


def test_parser_errors_and_defaults(capsys):
    import video_transfer as vt
    parser = vt.build_parser()
    base = ["--video", "clip", "--style", "s.png"]

    def check(argv):
        args = parser.parse_args(argv)
        vt.check_seg_args(parser, args)
        vt.check_window_args(parser, args)
        vt.check_stats_args(parser, args)
        return args
    a = check(base)
    assert (a.stats_window, a.stats_decay, a.stats_cut, a.map_drift) == (1, 1.0, 0.0, False)
    a = check(base + ["--stats_window", "8", "--stats_decay", "0.5", "--stats_cut", "0.01", "--map_drift"])
    assert (a.stats_window, a.stats_decay, a.stats_cut, a.map_drift) == (8, 0.5, 0.01, True)
    assert check(base + ["--map_drift"]).map_drift                      # any window
    a = check(base + ["--stats_window", "2", "--content_seg", "c.png", "--style_seg", "s_seg.png"])     # the static-mask route
    assert a.stats_window == 2

    def fails(argv, text):
        with pytest.raises(SystemExit) as e:
            check(base + argv)
        err = capsys.readouterr().err
        assert e.value.code == 2 and text in err, err
    for bad in ("0", "9", "-1"):
        fails(["--stats_window", bad], "--stats_window must be in 1..8")
    for bad in ("0", "1.5", "-0.1", "nan"):
        fails(["--stats_window", "3", "--stats_decay", bad], "--stats_decay must be in (0, 1]")
    for bad in ("-1", "nan", "inf"):
        fails(["--stats_window", "3", "--stats_cut", bad], "--stats_cut must be >= 0")
    fails(["--stats_window", "3", "--content_seg_dir", "maps", "--style_seg", "s_seg.png"], "not with --content_seg_dir or --auto_seg")
    fails(["--stats_window", "3", "--auto_seg", "--synthetic_seg_weights", "--no_seg_remap"], "not with --content_seg_dir or --auto_seg")
    fails(["--stats_decay", "0.5"], "belong to --stats_window")
    fails(["--stats_cut", "0.01"], "belong to --stats_window")
    fails(["--stats_window", "1", "--stats_cut", "0"], "belong to --stats_window")
    assert "No recommended value has been measured on real footage" in " ".join(parser.format_help().split())


def test_warmup_is_the_window_before_the_shard():
    from video_transfer import warmup_range
    assert warmup_range(4, 3) == (2, 3) and warmup_range(1, 3) == (0,) and warmup_range(0, 8) == ()


@pytest.fixture(scope="module")
def lib():
    from vstnet_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_library_exports_the_pool_entry(lib):
    from vstnet_amd import _lib
    from vstnet_amd.cwct import cWCT
    hdr = open(os.path.join(REPO, "include", "vstnet.h")).read()
    assert re.search(r"\bint\s+vst_cwct_stats_pool\s*\(", hdr) and "vst_cwct_stats_pool" in _lib.EXPORTS
    assert "Statistics window (version 113" in hdr
    assert hasattr(lib, "vst_cwct_stats_pool") and lib.vst_version() >= 113
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT vst_cwct_stats_pool\b", out)
    m = re.search(r"#define\s+VST_STATS_POOL_MAX\s+(\d+)", hdr)
    assert m and int(m.group(1)) == _lib.STATS_POOL_MAX == R.MAX_AGES == 8
    m = re.search(r"#define\s+VST_KERNEL_CWCT_POOL\s+(\d+)", hdr)
    assert m and int(m.group(1)) == _lib.KERNEL_CWCT_POOL and _lib.MISC_KERNELS[_lib.KERNEL_CWCT_POOL] == "cwct_pool"
    assert callable(cWCT.pool_stats) and callable(cWCT.frame_stats)
    table = open(_lib.RESOURCES_PATH).read() if os.path.exists(_lib.RESOURCES_PATH) else ""
    for line in table.splitlines():                          # (the table is written by a build; a prebuilt library has none)
        if "cwct_stats_pool_kernel" in line and "ScratchSize" in line:
            assert line.rstrip().endswith(": 0"), line


def test_pool_argument_errors_come_before_any_launch(lib):
    """No GPU here: every one of these returns before it touches the device."""
    for name, status, a in R.pool_error_cases():
        assert lib.vst_cwct_stats_pool(*a, None) == status, name


def test_cut_separation():
    """The margin the GPU cut and drift tests rely on, with the oracle encoder on the CPU: near-duplicate frames lie under T / 4,
    the two scenes over 4 T from each other, in both directions."""
    import torch
    from oracle import cpu_ref
    from vstnet_amd.synth import synthetic_state_dict
    sd = synthetic_state_dict(1234)
    A, B = R.scenes_u8(48, 64)

    def record(u8):
        x = torch.from_numpy(u8.astype(np.float32) / 255.0).permute(2, 0, 1)[None]
        with torch.no_grad():
            z = cpu_ref.revnet_forward(x, sd, 2)
        return stats64(z[0].reshape(z.shape[1], -1).numpy())
    ra, rb, rn = record(A), record(B), record(R.noisy_u8(A, seed=5))
    N = R.width_of(ra.shape[0])
    rel = lambda x, y: float(np.divide(*R.cut_distance(x, y, N)))      # noqa: E731
    near, ab, ba = max(rel(rn, ra), rel(ra, rn)), rel(rb, ra), rel(ra, rb)
    print(f"cut distance / tr(C_0): A vs A + noise {near:.3g}; B vs A {ab:.3g}; A vs B {ba:.3g}; T = {R.CUT_T}")
    assert near < R.CUT_T / 4
    assert ab > 4 * R.CUT_T and ba > 4 * R.CUT_T
