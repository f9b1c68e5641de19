"""numpy model of the band scan (include/sdrx.h "Band scan") for the tests: the yardstick, since the reference has no
counterpart.  Everything is defined bit for bit, so the model is compared with the device without a tolerance.

* :func:`cells` -- the cell sums in display order, added LEFT TO RIGHT (a loop over the w columns, vectorised across cells;
  ``np.sum`` adds pairwise and gives other bits).
* :func:`floor` -- the cell whose 64-bit pattern is the k-th smallest.
* :func:`evaluate` -- steps 3-7 on an integrated spectrum: (record fields, hits, cells).
* :class:`Integrator` -- frame by frame, with the no-observation rule.
* the inputs of tests/test_gpu_scan.py, so that tests/test_scan_model.py can check the conditions on them without a GPU.
"""
from __future__ import annotations

import numpy as np

N = 8192
MAX_HITS = 512
RECORD_KEYS = ("frame", "floor", "thr", "n_hits", "n_stored", "n_hot", "integrated", "frames", "cell_bins", "measured", "complete")


def cfg(cell_bins, frames=1, floor_permille=500, ratio_q8=256, min_cells=1) -> dict:
    return dict(cell_bins=cell_bins, frames=frames, floor_permille=floor_permille, ratio_q8=ratio_q8, min_cells=min_cells)


def cells(acc: np.ndarray, w: int) -> np.ndarray:
    """cell[c] = ((a0 + a1) + a2) + ... over display bins c w .. c w + w - 1; display bin b = natural bin (b + N/2) mod N"""
    acc = np.asarray(acc, np.float64)
    assert acc.shape == (N,)
    display = np.concatenate([acc[N // 2:], acc[:N // 2]]).reshape(N // w, w)
    out = display[:, 0].copy()
    for j in range(1, w):
        out = out + display[:, j]
    return out


def rank(q: int, C: int) -> int:
    return (q * (C - 1)) // 1000


def floor(cell: np.ndarray, q: int) -> np.float64:
    """the cell whose pattern, read as an unsigned integer, is the k-th smallest (equal ones each count)"""
    pat = np.sort(np.ascontiguousarray(cell, np.float64).view(np.uint64))
    return pat[rank(q, cell.size):rank(q, cell.size) + 1].view(np.float64)[0]


def runs(hot: np.ndarray) -> list[tuple[int, int]]:
    """[(first, last)] of the maximal runs of True inside 0 .. C - 1: no wrap"""
    edge = np.diff(np.concatenate([[0], hot.astype(np.int8), [0]]))
    return list(zip(np.nonzero(edge == 1)[0].tolist(), (np.nonzero(edge == -1)[0] - 1).tolist()))


def evaluate(acc: np.ndarray, c: dict):
    """(fields, hits, cells): floor, thr, n_hits, n_stored, n_hot; every hit (not only the stored ones) as a dict; the cells"""
    cell = cells(acc, c["cell_bins"])
    fl = floor(cell, c["floor_permille"])
    with np.errstate(invalid="ignore", over="ignore"):
        thr = np.float64(fl) * (np.float64(c["ratio_q8"]) / np.float64(256.0))
        hot = cell > thr
    hits = []
    for first, last in runs(hot):
        n = last - first + 1
        if n < c["min_cells"]:
            continue
        peak = first + int(np.argmax(cell[first:last + 1]))  # (the first of the largest; a hot cell is no NaN)
        hits.append(dict(first_cell=first, n_cells=n, peak_cell=peak, peak_pwr=float(cell[peak])))
    fields = dict(floor=float(fl), thr=float(thr), n_hits=len(hits), n_stored=min(len(hits), MAX_HITS), n_hot=int(hot.sum()))
    return fields, hits, cell


class Integrator:
    """One source's scan, frame by frame.  ``step(psd, frame)`` with the PSD of a frame in which the source was measured, or None
    for a frame in which it was not (no observation: count and ACC stay); returns that frame's record.  ``hits`` (the stored
    ones), ``cells`` and ``eval_frame`` are those of the last completed evaluation."""

    def __init__(self, c: dict):
        self.c = dict(c)
        self.acc = np.zeros(N, np.float64)
        self.count = 0
        self.hits, self.cells, self.eval_frame = None, None, None

    def step(self, psd, frame: int) -> dict:
        rec = dict.fromkeys(RECORD_KEYS, 0)
        rec.update(frame=frame, floor=0.0, thr=0.0)
        if psd is None or self.c["cell_bins"] == 0:
            return rec
        psd = np.asarray(psd, np.float64)
        self.acc = psd.copy() if self.count == 0 else self.acc + psd
        self.count += 1
        rec.update(integrated=self.count, frames=self.c["frames"], cell_bins=self.c["cell_bins"], measured=1)
        if self.count == self.c["frames"]:
            fields, hits, cell = evaluate(self.acc, self.c)
            rec.update(fields, complete=1)
            self.hits, self.cells, self.eval_frame = hits[:MAX_HITS], cell, frame
            self.count = 0
        return rec


# ---- the inputs of the GPU tests (tests/test_gpu_scan.py), built here so that tests/test_scan_model.py can check the
# ---- conditions on them without a GPU
WT_SEEDS = (30, 31, 32)                    # three raw frames of watch_ref.watch_tree(): drift_ref.wt_frame, one tone per USB sub
WT_CARRIERS = cfg(4, floor_permille=500, ratio_q8=16 * 256)  # gives exactly the eight tones (frames = 1 and 3)
WT_NOISE = cfg(1, floor_permille=500, ratio_q8=4 * 256)      # several hundred noise hits: exercises the list
WT_TRUNCATED = cfg(1, floor_permille=500, ratio_q8=256)      # more than MAX_HITS hits
WT_LEAF = 1                                # a leaf of the main's stream
PARKED_SUB, PARKED_OFF_HZ = 3, 7000.0      # the end-to-end test: this sub is parked and mistuned by +7 kHz


def wt_frames(topo) -> list[np.ndarray]:
    import drift_ref as dr
    return [dr.wt_frame(topo, 0.0, seed=s, start=f * topo.frame) for f, s in enumerate(WT_SEEDS)]


def wt_tone_cells(topo, w: int) -> list[int]:
    """the cell of the parent's spectrum that holds the tone of each USB sub 1 .. 8 of watch_tree()"""
    import watch_ref as wr
    fs_parent = topo.vfos[1].fs
    out = []
    for k in range(1, 9):
        hz = wr.tone_for(topo, k) + topo.vfos[0].mixer_freq
        out.append((int(round(hz * N / fs_parent)) + N // 2) // w)
    return out


def edge_tone_frame(topo) -> np.ndarray:
    """drift_tree's raw frame with one tone at -fs/2: integer components (-100 .. 100, so that it can be fed as bytes), a tone of
    amplitude 60 alternating in sign, +-2 of noise.  The Hann window spreads it over the bins N/2 - 1, N/2 and N/2 + 1 (natural):
    display bins N - 1, 0 and 1 -- the last cell and the first."""
    rng = np.random.default_rng(77)
    n = topo.frame
    z = 60.0 * np.where(np.arange(n) % 2 == 0, 1.0, -1.0) + 0j
    z = z + 2.0 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    x = np.ascontiguousarray(z.astype(np.complex64)).view(np.float32)
    return np.clip(np.rint(x), -100, 100).astype(np.float32)
