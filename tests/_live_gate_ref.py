"""A sequential numpy model of the live frames' motion gate, written from the rule of include/advhip.h ("live frames: motion
gate") alone, so that the device kernels and live.gate_decision have something independent to equal:

    per pushed frame f of camera c: n = #{i : |f[i] - anchor[i]| > tau} on int16 differences;
    still == -1 or n > limit: MOVES -- anchor := f, still := 0, epoch += 1, peak := 0, changed := n (or -1 without an anchor);
    else STILL -- still := min(still + 1, 2^30), changed := n, peak := max(peak, n);
    a due window of span R is QUIET iff still + 1 >= R;
    a quiet window is HELD iff ref_epoch == epoch and (max_hold is None or holds < max_hold), then holds += 1; an extracted quiet
    window: ref_epoch := epoch, holds := 0; an extracted window that is not quiet: ref_epoch := None, holds := 0;
    reset: still := -1, epoch += 1, ref_epoch := None, holds := 0."""
import numpy as np

STILL, EPOCH, CHANGED, PEAK = range(4)
INIT = (-1, 0, -1, 0)


def changed_bytes(f, a, tau):
    d = f.astype(np.int16).ravel() - a.astype(np.int16).ravel()
    return int((np.abs(d) > tau).sum())


def changed_bytes_scalar(f, a, tau):
    """The same count by a per-byte loop on Python ints (tiny frames only)."""
    n = 0
    for x, y in zip(f.ravel().tolist(), a.ravel().tolist()):
        d = x - y
        if d > tau or -d > tau:
            n += 1
    return n


class MotionGateRef:
    def __init__(self, n_cam, frame_shape, tau, limit, span=1, max_hold=None, anchor_fill=0):
        self.n_cam, self.frame_shape, self.tau, self.limit, self.span, self.max_hold = n_cam, tuple(frame_shape), tau, limit, span, max_hold
        self.anchor = np.full((n_cam,) + self.frame_shape, anchor_fill, dtype=np.uint8)
        self.state = np.tile(np.array(INIT, dtype=np.int32), (n_cam, 1))
        self.ref_epoch = [None] * n_cam
        self.holds = [0] * n_cam

    def push(self, cams, frames, count=changed_bytes):
        """One frame per listed camera -> [moves] per listed camera; ids outside [0, n_cam) are skipped as the kernels skip them."""
        frames = np.asarray(frames, dtype=np.uint8)
        assert frames.shape == (len(cams),) + self.frame_shape
        verdicts = []
        for i, c in enumerate(cams):
            if not 0 <= c < self.n_cam:
                verdicts.append(None)
                continue
            st = self.state[c]
            n = count(frames[i], self.anchor[c], self.tau)
            if st[STILL] == -1 or n > self.limit:
                st[CHANGED] = -1 if st[STILL] == -1 else n
                self.anchor[c] = frames[i]
                st[STILL], st[PEAK] = 0, 0
                st[EPOCH] += 1
                verdicts.append(True)
            else:
                st[STILL] = min(int(st[STILL]) + 1, 1 << 30)
                st[CHANGED] = n
                st[PEAK] = max(int(st[PEAK]), n)
                verdicts.append(False)
        return verdicts

    def quiet(self, c):
        return int(self.state[c, STILL]) + 1 >= self.span

    def decide(self, due):
        """-> (extract, held) in `due` order, the bookkeeping committed."""
        extract, held = [], []
        for c in due:
            held_c, self.ref_epoch[c], self.holds[c] = decision(int(self.state[c, STILL]), int(self.state[c, EPOCH]), self.span, self.ref_epoch[c],
                                                                self.holds[c], self.max_hold)
            (held if held_c else extract).append(c)
        return tuple(extract), tuple(held)

    def reset(self, cams):
        for c in cams:
            self.state[c, STILL] = -1
            self.state[c, EPOCH] += 1
            self.ref_epoch[c], self.holds[c] = None, 0


def decision(still, epoch, span, ref_epoch, holds, max_hold):
    """(held, ref_epoch, holds) after the decision for one due window, in the rule's own words."""
    quiet = still + 1 >= span
    if quiet:
        if ref_epoch == epoch and (max_hold is None or holds < max_hold):
            return True, ref_epoch, holds + 1
        return False, epoch, 0
    return False, None, 0


def off_positions(frame_bytes, chunk, width, k):
    """k distinct byte positions of a frame, the places a kernel can go wrong first: byte 0, the last byte, both sides of the
    chunk boundary (where the frame has one), inside the last vector of `width` bytes; then the rest ascending.  `chunk` and
    `width` may be tuples: the places of several access widths."""
    assert 0 <= k <= frame_bytes
    chunks, widths = (chunk if isinstance(chunk, tuple) else (chunk,)), (width if isinstance(width, tuple) else (width,))
    first = [0, frame_bytes - 1] + [p for ch in chunks for p in (ch - 1, ch)] + [p for w in widths for p in (frame_bytes - w, frame_bytes - (w + 1) // 2)]
    order, seen = [], set()
    for p in first + list(range(frame_bytes)):
        if len(order) == k:
            break
        if 0 <= p < frame_bytes and p not in seen:
            order.append(p)
            seen.add(p)
    assert len(order) == k
    return order


def anchor_with_room(rng, shape, delta):
    """A frame every byte of which can move by `delta` and stay a byte: random in [delta, 255 - delta] while both directions
    fit, else 0 at even and 255 at odd positions (one direction each, so that both signs still occur)."""
    n = int(np.prod(shape))
    if 2 * delta <= 255:
        a = rng.integers(delta, 256 - delta, size=n, dtype=np.int64)
    else:
        a = np.where(np.arange(n) % 2 == 0, 0, 255)
    return a.astype(np.uint8).reshape(shape)


def frame_off_by(anchor, positions, delta):
    """`anchor` with the bytes at `positions` moved by exactly `delta` (alternating signs; the sign that stays inside [0, 255]
    where only one does) -- the caller chooses an anchor with room on both sides where it can."""
    f = anchor.copy().ravel().astype(np.int16)
    for j, p in enumerate(positions):
        sign = 1 if j % 2 == 0 else -1
        if not 0 <= f[p] + sign * delta <= 255:
            sign = -sign
        f[p] += sign * delta
        assert 0 <= f[p] <= 255, (p, delta)
    return f.astype(np.uint8).reshape(anchor.shape)
