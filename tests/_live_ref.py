"""A numpy model of the live scorer's state (anomaly_detection_on_video_amd/live.py): per-camera rings of the last W clips with
the magnitude channel np.linalg.norm(x, axis=-1) appended, and the windows a padded batch is filled with.  Written from the
slot rule alone -- the clip pushed at count k lies in slot k % W -- so that the device kernels have something independent to
equal bit for bit."""
import numpy as np


class RingRef:
    def __init__(self, n_cam, ncrops, W, C):
        self.n_cam, self.ncrops, self.W, self.C = n_cam, ncrops, W, C
        self.ring = np.zeros((n_cam, ncrops, W, C + 1), dtype=np.float32)
        self.counts = np.zeros((n_cam,), dtype=np.int64)

    def push(self, cams, feats):
        """feats (len(cams), ncrops, C) float32: one new clip per listed camera."""
        feats = np.asarray(feats, dtype=np.float32)
        assert feats.shape == (len(cams), self.ncrops, self.C) and len(set(cams)) == len(cams)
        for i, c in enumerate(cams):
            slot = int(self.counts[c] % self.W)
            self.ring[c, :, slot, :self.C] = feats[i]
            self.ring[c, :, slot, self.C] = np.linalg.norm(feats[i], axis=-1)
            self.counts[c] += 1

    def lens(self, cams, tmax=None):
        tmax = self.W if tmax is None else tmax
        return [int(min(self.counts[c], self.W, tmax)) for c in cams]

    def windows(self, cams, tmax, fill=np.nan):
        """(len(cams), ncrops, tmax, C + 1): camera cams[v]'s last len clips, oldest first, `fill` behind them."""
        dst = np.full((len(cams), self.ncrops, tmax, self.C + 1), fill, dtype=np.float32)
        for v, (c, n) in enumerate(zip(cams, self.lens(cams, tmax))):
            k = int(self.counts[c])
            for t in range(n):
                dst[v, :, t] = self.ring[c, :, (k - n + t) % self.W]
        return dst


def scripted_counts(W):
    """The counts the tests' push sequence leaves six cameras at."""
    return [0, 1, W - 1, W, W + 1, 2 * W + 3]


def scripted_pushes(W, ncrops, C, seed=0, spread=3.0):
    """[(cams, feats)]: step s pushes one clip to every camera whose target count (scripted_counts) is above s -- all but camera 0
    at first, ever smaller subsets later.  A row is normal noise times exp(uniform(-spread, spread)): rows of very different magnitude."""
    target = scripted_counts(W)
    rng = np.random.default_rng(1234 + 97 * W + C + seed)
    steps = []
    for s in range(max(target)):
        cams = [c for c, k in enumerate(target) if k > s]
        feats = (rng.standard_normal((len(cams), ncrops, C)) * np.exp(rng.uniform(-spread, spread, (len(cams), ncrops, 1)))).astype(np.float32)
        steps.append((cams, feats))
    return steps
