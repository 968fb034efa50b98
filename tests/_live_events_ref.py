"""The streaming event rule (include/advhip.h: live events; events.LiveEventTracker) restated sequentially for ONE camera: one
sample per call, fp32 arithmetic through np.float32, the float64 sum as Python floats, alert and open_start after every call,
finish and reset.  It keeps the whole series in a list, not a ring, and reads windows out of it by position: independent of the
kernel's ring and of the offline references (tests/_events_ref.py), against which test_live_events_host checks it."""
import numpy as np


class LiveRef:
    def __init__(self, low, high, smooth=1, merge_gap=0, min_len=1):
        self.low, self.high = np.float32(low), np.float32(high)
        self.h, self.gap, self.min_len = (smooth - 1) // 2, merge_gap, min_len
        self.generation = 0
        self.events = []   # (generation, start, end, peak_frame, peak fp32, mean fp32), in emission order, over all generations
        self.emit_at = []  # the sample count at which each was emitted (None: by finish)
        self._clear()

    def _clear(self):
        self.x, self.start = [], -1
        self.alert, self.open_start = 0, -1

    @property
    def samples(self):
        return len(self.x)

    def _mean(self, lo, hi):
        acc = np.float32(0.0)
        with np.errstate(invalid="ignore", over="ignore"):
            for u in range(lo, hi + 1):
                acc = np.float32(acc + self.x[u])
            return np.float32(acc / np.float32(hi - lo + 1))

    def _close(self, at):
        end = self.last + 1
        if self.strong and end - self.start >= self.min_len:
            with np.errstate(invalid="ignore", over="ignore"):
                mean = np.float32(self.snap / (end - self.start))
            self.events.append((self.generation, self.start, end, self.peak_at, self.peak, mean))
            self.emit_at.append(at)
        self.start = -1

    def _step(self, t, y, at):
        active = bool(y >= self.low)
        if self.start >= 0:
            self.run += float(y)
            if active:
                self.last, self.snap = t, self.run
                self.strong = self.strong or bool(y >= self.high)
                if y > self.peak:
                    self.peak, self.peak_at = y, t
            elif t - self.last > self.gap:
                self._close(at)
        elif active:
            self.start = self.last = self.peak_at = t
            self.strong, self.peak = bool(y >= self.high), y
            self.run = 0.0 + float(y)
            self.snap = self.run

    def _flags(self):
        self.alert = int(self.start >= 0 and self.strong and self.last + 1 - self.start >= self.min_len)
        self.open_start = self.start

    def update(self, sample):
        self.x.append(np.float32(sample))
        n = len(self.x)
        t = n - 1 - self.h
        if t >= 0:
            self._step(t, self._mean(max(0, t - self.h), n - 1), n)
        self._flags()

    def finish(self):
        n = len(self.x)
        for t in range(max(0, n - self.h), n):
            self._step(t, self._mean(max(0, t - self.h), n - 1), None)
        if self.start >= 0:
            self._close(None)
        self.reset()

    def reset(self):
        self._clear()
        self.generation += 1


def rows(events):
    """[(generation, start, end, peak_frame, peak, mean)] -> (int32 (E, 4), fp32 (E, 2))"""
    return (np.asarray([e[:4] for e in events], dtype=np.int32).reshape(-1, 4), np.asarray([e[4:] for e in events], dtype=np.float32).reshape(-1, 2))
