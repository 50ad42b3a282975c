"""vstnet_amd.pipeline.WindowRing on the host: the class the frame loop's logit ring and record rings run on, driven with fake
events and streams through FramePipeline.run's schedule - submit frame t, then retire frame t - (depth - 1) once depth - 1 newer
frames are queued; warm-up frames claim and publish and are never retired."""
import pytest

from vstnet_amd.pipeline import WindowRing, logit_ring_slots

N_FRAMES = 50


class FakeStream:
    """The stream of one frame: lists the frames whose events it was told to wait for."""

    def __init__(self, frame):
        self.frame, self.waited = frame, []

    def wait_event(self, event):
        self.waited.append(event.by)


class FakeEvent:
    """Remembers the frame whose stream recorded it last."""

    def __init__(self):
        self.by = None

    def record(self, stream):
        self.by = stream.frame


def replay(window, depth, start, n_warm, behind=0):
    """run()'s schedule over N_FRAMES frames from frame `start`, after n_warm warm-up frames; retirement is held `behind` frames
    further back than run() holds it.  Checks what every gather returns and waits for."""
    ring = WindowRing(window, depth, FakeEvent)
    assert ring.slots == logit_ring_slots(window, depth) == window + depth and len(ring.ready) == ring.slots
    first = start - n_warm
    ring.start(first)
    holds, last_retired = [None] * ring.slots, None
    for i in range(first, start):                       # warm-up: written and signalled, never retired
        j = ring.claim(i, last_retired)
        assert j == i % ring.slots
        holds[j] = i
        ring.publish(i, FakeStream(i))
    lag, n = depth - 1, 0
    for i in range(start, start + N_FRAMES):
        stream = FakeStream(i)
        j = ring.claim(i, last_retired)
        assert j == i % ring.slots
        holds[j] = i
        ring.publish(i, stream)
        assert ring.ready[j].by == i
        order = ring.gather(i, stream)
        ages = min(window, i - first + 1)
        assert len(order) == ages and order[0] == j, (window, depth, start, n_warm, i)
        assert [holds[s] for s in order] == [i - a for a in range(ages)], (window, depth, start, n_warm, i)
        assert stream.waited == [i - a for a in range(1, ages)], (window, depth, start, n_warm, i)
        n += 1
        if n > lag + behind:
            last_retired = start + n - 1 - lag - behind


def grid(window):
    for depth in range(2, 7):
        for start in (0, 5):
            for n_warm in range(min(window - 1, start) + 1):
                yield depth, start, n_warm


@pytest.mark.parametrize("window", range(1, 9))
def test_ring_under_the_frame_loop_schedule(window):
    for depth, start, n_warm in grid(window):
        replay(window, depth, start, n_warm)


@pytest.mark.parametrize("window", range(1, 9))
def test_one_frame_behind_is_the_spare_slot(window):
    """R = window + depth keeps one slot to spare: retirement one frame further behind still never meets a live reader."""
    for depth, start, n_warm in grid(window):
        replay(window, depth, start, n_warm, behind=1)


@pytest.mark.parametrize("window", range(1, 9))
def test_two_frames_behind_trips_the_assertion(window):
    """Two frames behind, a write meets an unretired reader - if and only if anybody reads an older slot at all."""
    for depth, start, n_warm in grid(window):
        if window >= 2:
            with pytest.raises(AssertionError, match=r"record slot \d+: frame \d+ may still read what frame \d+ is about to overwrite"):
                replay(window, depth, start, n_warm, behind=2)
        else:
            replay(window, depth, start, n_warm, behind=2)


def test_start_clears_the_readers():
    """A run is one history: the readers an earlier run left are nobody's once the next run starts."""
    ring = WindowRing(3, 2, FakeEvent, what="logit")
    ring.start(0)
    for i in range(3):
        ring.claim(i, None)
        ring.publish(i, FakeStream(i))
        ring.gather(i, FakeStream(i))
    assert ring.reader[:2] == [2, 2]
    with pytest.raises(AssertionError, match="logit slot 0: frame 2 may still read what frame 5 is about to overwrite"):
        ring.claim(5, 1)
    ring.start(5)
    assert ring.reader == [None] * ring.slots and ring.claim(5, None) == 0
    assert ring.gather(5, FakeStream(5)) == [0]          # the run's first frame: a window of one
