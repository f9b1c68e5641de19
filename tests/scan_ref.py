"""numpy model of the band scan (include/sdrx.h "Band scan") for the tests: the yardstick, since the reference has no
counterpart.  Everything is defined bit for bit, so the model is compared with the device without a tolerance.

* :func:`cells` -- the cell sums in display order, added LEFT TO RIGHT (a loop over the w columns, vectorised across cells;
  ``np.sum`` adds pairwise and gives other bits).
* :func:`floor` -- the cell whose 64-bit pattern is the k-th smallest.
* :func:`evaluate` -- steps 3-7 on an integrated spectrum: (record fields, hits, cells).
* :class:`Integrator` -- frame by frame, with the no-observation rule.
* the inputs of tests/test_gpu_scan.py, so that tests/test_scan_model.py can check the conditions on them without a GPU.
* the crafted inputs of tests/test_gpu_scan_crafted.py (comb, all hot, ruler, spread comb, 512 / 513 hits), likewise.
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


# ---- the crafted inputs of tests/test_gpu_scan_crafted.py: spectra designed so that the radix select meets ties and the
# ---- segmented scan meets runs that cross threads and waves.  The source is the raw frame of drift_ref.drift_tree(8704):
# ---- 69 632 samples, S = 8 segments of 8192 at stride 8704.  The SAME segment is written at each of the eight starts, so the
# ---- PSD is a sum of eight equal fp32 values -- exactly 8 x the segment's power -- and bit-equal bins stay bit-equal.
# ---- tests/test_scan_model.py asserts every condition named here on the model, tests/test_gpu_scan_crafted.py on the device.
CR_PARENT = 8704
THREADS = 512                                   # of k_watch_scan: thread t owns the cells t P .. t P + P - 1, a wave 64 P
WIDTHS = (1, 2, 4, 8, 16, 32, 64, 128, 256)


def per_thread(w: int) -> int:
    """P: the cells a thread of the run scan owns at cell width w (a wave owns 64 P)"""
    return max(N // w // THREADS, 1)


def crafted_tree():
    import drift_ref as dr
    return dr.drift_tree(CR_PARENT)


def repeated(topo, seg: np.ndarray) -> np.ndarray:
    """the raw frame (interleaved float32) with the 8192-sample complex segment at each of the watch's segment starts, zeros
    between them"""
    import drift_ref as dr
    import watch_ref as wr
    S, starts = wr.segments(topo.frame)
    seg = np.asarray(seg, np.complex64)
    assert seg.shape == (N,) and S == 8 and starts[1] - starts[0] >= N
    z = np.zeros(topo.frame, np.complex64)
    for st in starts:
        z[st:st + N] = seg
    return dr.interleaved(z)


def _from_spectrum(X: np.ndarray) -> np.ndarray:
    """the segment whose (unwindowed) transform is X, natural order"""
    return np.fft.ifft(X).astype(np.complex64)


def _natural(display) -> np.ndarray:
    return (np.asarray(display) + N // 2) % N


def _floor_spectrum(seed: int) -> np.ndarray:
    """unit magnitude, random phase in every bin"""
    rng = np.random.default_rng(seed)
    return np.exp(2j * np.pi * rng.random(N))


# a. two impulses half a segment apart: the even natural bins share one bit pattern, the odd ones another
COMB_LOW_Q, COMB_HIGH_Q = (499, 500), 501        # rank(500, 8192) = 4095 is the last low cell, rank(501, 8192) = 4103 a high one
COMB_RATIO_Q8 = 512


def comb_frame(topo) -> np.ndarray:
    seg = np.zeros(N, np.complex64)
    seg[2048] = seg[6144] = 64.0
    return repeated(topo, seg)


# b. everything hot: the threshold is the smallest cell / 256, one run over all C cells whose peak is the argmax
ALL_HOT_SEED = 1
ALL_HOT_PEAKS = {1: 3727, 4: 931, 16: 226, 256: 14}


def all_hot_frame(topo) -> np.ndarray:
    import drift_ref as dr
    return dr.raw_frame(topo, 0.0, seed=ALL_HOT_SEED)


def all_hot_cfg(w: int, min_cells: int = 1) -> dict:
    return cfg(w, floor_permille=0, ratio_q8=1, min_cells=min_cells)


# c. the ruler: plateaus at chosen display cells over a unit noise floor
RULER_A = 100.0          # the plateau's amplitude: 8 A^2 = 80 000 in the PSD; the skirt bin beside a plateau has 8 A^2 / 16 = 5 000,
RULER_BOOST = 2.0        # a plateau's own edge bin 8 x 9 A^2 / 16 = 45 000; the floor's bins lie below 8
RULER_Q = 250            # fewer than three quarters of the cells are hot: the floor is a noise cell
RULER_THR = 16000.0      # where the threshold is aimed: between the skirt (5 000 + noise) and the edge (45 000 - noise)
RULER_RATIO_Q8 = 1896152  # at w = 1: 16 000 / the floor the model finds there (2.16); the floor grows with w, so w divides it
RULER2_RATIO_Q8 = 770771  # the same for the sum of the two frames of ruler2_frames (floor 5.31)
RULER_WIDTHS = (1, 2, 4, 8, 16)  # the widths with a ruler of their own: C >= 512, every thread owns P = C / 512 cells
RULER_WIDE = 16           # the wider cells (fewer cells than threads: whole waves own nothing) look at this width's ruler


def ruler_runs(w: int) -> dict:
    """{name: (first, last)} in cells of width w, laid out on the thread (P cells) and wave (64 P cells) grid of that width"""
    P = per_thread(w)
    W, C = 64 * P, N // w
    assert C == 8 * W
    return dict(begins_at_0=(0, 1),
                one_thread=(3 * P, 4 * P - 1),
                thread_straddle=(6 * P - 1, 6 * P),
                wave_straddle=(W - 1, W),
                wave_first=(2 * W, 2 * W + 2),
                wave_last=(3 * W - 3, 3 * W - 1),
                three_waves=(3 * W + 40 * P + P // 2, 7 * W + 2 * P + P // 2 - (1 if P > 1 else 0)),
                ends_at_last=(C - 2, C - 1))


def ruler_boosted_cell(w: int) -> int:
    """the cell of the three-wave run that is raised: in the middle one of the waves the run covers whole"""
    P = per_thread(w)
    return 5 * 64 * P + 21 * P + P // 2


def ruler_frame(topo, w: int, seed: int = 5, runs=None) -> np.ndarray:
    """Plateaus over the display bins of `runs` (default :func:`ruler_runs`, cells of w bins).  X[k] = A (-1)^k on a plateau's
    natural bins: the Hann window's three taps (-1/4, 1/2, -1/4) then add up and the plateau is flat.  One bin of the cell
    :func:`ruler_boosted_cell` carries RULER_BOOST x A."""
    runs = ruler_runs(w) if runs is None else runs
    X = _floor_spectrum(seed)
    sign = np.where(np.arange(N) % 2 == 0, 1.0, -1.0)
    for first, last in runs.values():
        k = _natural(np.arange(first * w, last * w + w))
        X[k] = RULER_A * sign[k]
    k = int(_natural(ruler_boosted_cell(w) * w + w // 2))
    X[k] = RULER_BOOST * RULER_A * sign[k]
    return repeated(topo, _from_spectrum(X))


def ruler_cfg(w: int, frames: int = 1, min_cells: int = 1) -> dict:
    ratio = (RULER_RATIO_Q8 if frames == 1 else RULER2_RATIO_Q8) // w
    return cfg(w, frames=frames, floor_permille=RULER_Q, ratio_q8=ratio, min_cells=min_cells)


def ruler_for(topo, w: int) -> np.ndarray:
    """the ruler frame cell width w is run on: its own up to 16 bins, that of 16 bins beyond"""
    return ruler_frame(topo, min(w, RULER_WIDE))


def ruler_conditions(hits: list[dict], w: int) -> dict:
    """What the ruler's hit list must contain, each as a bool -- from the HITS alone (the design is not consulted): the thread and
    wave geometry of cell width w."""
    P = per_thread(w)
    W, C = 64 * P, N // w
    span = [(h["first_cell"], h["first_cell"] + h["n_cells"] - 1, h["peak_cell"]) for h in hits]
    out = dict(
        wave_straddle=any(b == a + 1 and b % W == 0 for a, b, _ in span),
        three_waves=any(b // W - a // W >= 4 and a // W < p // W < b // W and (P == 1 or (a % P != 0 and b % P != P - 1)) for a, b, p in span),
        wave_first=any(a % W == 0 and a > 0 for a, b, _ in span),
        wave_last=any(b % W == W - 1 and b < C - 1 for a, b, _ in span),
        begins_at_0=any(a == 0 for a, b, _ in span),
        ends_at_last=any(b == C - 1 for a, b, _ in span),
        no_wrap=sum(1 for a, b, _ in span if a == 0 or b == C - 1) == 2)
    if P > 1:
        out.update(one_thread=any(a % P == 0 and b == a + P - 1 for a, b, _ in span),
                   thread_straddle=any(b == a + 1 and b % P == 0 and b % W != 0 for a, b, _ in span))
    return out


def wide_conditions(hits: list[dict], w: int) -> dict:
    """w > 16 on the ruler of 16 bins: the ends stay two hits, and the long run (7 008 bins) is still the widest by far"""
    C = N // w
    return dict(begins_at_0=hits[0]["first_cell"] == 0, ends_at_last=hits[-1]["first_cell"] + hits[-1]["n_cells"] == C,
                two_hits_at_the_ends=len(hits) >= 3, long_run=max(h["n_cells"] for h in hits) * w >= 3 * 1024)


def second_longest_plus_one(hits: list[dict]) -> int:
    return sorted(h["n_cells"] for h in hits)[-2] + 1


# the multi-frame ruler: two DIFFERENT frames, M = 2 at w = 1 -- ACC is their sum, and the runs are those of the sum
RULER2_W = 1


def ruler2_frames(topo) -> list[np.ndarray]:
    """the ruler of w = 1 split over two frames: each carries every second plateau over a noise floor of its own, so the ruler's
    runs appear only in the sum"""
    runs = ruler_runs(RULER2_W)
    names = sorted(runs)
    a = {k: runs[k] for k in names[0::2]}
    b = {k: runs[k] for k in names[1::2]}
    return [ruler_frame(topo, RULER2_W, seed=6, runs=a), ruler_frame(topo, RULER2_W, seed=7, runs=b)]


# d. one tone every L bins: N / L hits at w = 1, spread evenly over the eight waves, the list not truncated
SPREAD_L = 32
SPREAD_CFG = cfg(1, floor_permille=500, ratio_q8=72 * 256)  # thr near 200: the tone (3 200) and its skirt (800) are hot, the noise (< 8) is not


def spread_comb_frame(topo, L: int = SPREAD_L, seed: int = 8) -> np.ndarray:
    X = _floor_spectrum(seed)
    X[L // 2::L] = 40.0  # (display bins L/2 + L j: none at the edge, every run of three straddles a thread boundary at L = 32)
    return repeated(topo, _from_spectrum(X))


# e. exactly MAX_HITS and MAX_HITS + 1 hits: Gaussian noise in the segment, two neighbouring ratios found by a search on the model
EDGE_SEED = 9
EDGE_512 = cfg(1, floor_permille=500, ratio_q8=879)
EDGE_513 = cfg(1, floor_permille=500, ratio_q8=878)
EDGE_FEW = cfg(1, floor_permille=500, ratio_q8=8 * 256)   # the evaluation before the 513-hit one: a handful of hits


def edge_noise_frame(topo, seed: int = EDGE_SEED) -> np.ndarray:
    rng = np.random.default_rng(seed)
    return repeated(topo, (rng.standard_normal(N) + 1j * rng.standard_normal(N)).astype(np.complex64))
