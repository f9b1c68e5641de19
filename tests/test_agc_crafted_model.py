"""The crafted AGC schedules of tests/agc_crafted_ref.py without a GPU: every case tests/test_gpu_agc_crafted.py relies on is
there -- counted on the model run, not on the plan -- and every wrong rule of ``mutants()`` that a call sequence can tell from
the right one gives another record on at least one scheduled (leaf, frame)."""
import numpy as np

import agc_crafted_ref as cr
from sdrreceiver_amd import agc


def _bits(x) -> int:
    return int(np.float32(x).view(np.uint32))


def _boundary_cases():
    return [c for name in cr.TREES for c in cr.cases(cr.boundary(name))]


def test_the_restated_rule_is_the_rule():
    """agc_crafted_ref.rule without a flaw gives agc.step's record on every scheduled case, and that is the record of the run."""
    for c in cr.all_cases():
        g2, q, a = agc.step(c["cfg"], c["q"], c["g"], c["meter"])
        assert cr.rule(c) == (_bits(g2), q, a) == (_bits(c["rec"]["gain_next"]), c["rec"]["quiet_run"], c["rec"]["action"]), c


def test_threshold_cases():
    """s == T n, T n + r and T n - r at least three times each for T = hi_ms, lo_ms and silent_ms, decided as the rule says;
    products of 2^32 and more; leaves with several meter records; hi_ms = 2^30; silent_ms == lo_ms."""
    cs = _boundary_cases()
    count = {}
    for c in cs:
        for t in cr.THRESHOLDS:
            rel = cr.relation(c, t)
            if rel:
                count[(t, rel)] = count.get((t, rel), 0) + 1
                kind, cfg = cr.kind_of(c), c["cfg"]
                if t == "hi_ms":
                    assert (kind == "hot") == (rel == "+r"), c
                elif t == "lo_ms" and cfg.silent_ms < cfg.lo_ms:
                    assert (kind == "cold") == (rel == "-r"), c
                elif t == "silent_ms" and cfg.silent_ms < cfg.lo_ms:
                    assert kind == ("silent" if rel == "-r" else "cold"), c
    print("threshold cases:", {f"{t} {r}": count.get((t, r), 0) for t in cr.THRESHOLDS for r in ("eq", "+r", "-r")})
    for t in cr.THRESHOLDS:
        for rel in ("eq", "+r", "-r"):
            assert count.get((t, rel), 0) >= 3, (t, rel, count)
    near = [c for c in cs if any(cr.relation(c, t) for t in cr.THRESHOLDS)]
    big = [c for c in near if any(cr.relation(c, t) and getattr(c["cfg"], t) * c["meter"]["n_values"] >= 1 << 32 for t in cr.THRESHOLDS)]
    big_eq = [c for c in big if any(cr.relation(c, t) == "eq" for t in cr.THRESHOLDS)]
    several = [c for c in near if c["meter"]["n_values"] >= 2048]
    top = [c for c in near if c["cfg"].hi_ms == cr.FULL]
    both = [c for c in near if c["cfg"].silent_ms == c["cfg"].lo_ms > 0 and cr.relation(c, "lo_ms")]
    print(f"T n >= 2^32: {len(big)} ({len(big_eq)} at equality); n_out >= 2048: {len(several)}; hi_ms = 2^30: {len(top)}; silent_ms == lo_ms: {len(both)}")
    assert len(big) >= 3 and len(big_eq) >= 1 and len(several) >= 3 and len(top) >= 1
    # silent_ms == lo_ms: equality is in the window, one below is silent -- never cold
    assert {cr.relation(c, "lo_ms") for c in both} >= {"eq", "-r"}
    for c in both:
        assert cr.kind_of(c) == {"eq": "window", "+r": "window", "-r": "silent"}[cr.relation(c, "lo_ms")], c


def test_zero_frames():
    """All-zero input gives s == 0: in the window with silent_ms = lo_ms = 0 (quiet_run 0), cold with lo_ms = 1 (and counted on
    in the frame that follows without a call), silent with silent_ms = 1."""
    seen = set()
    for name in cr.TREES:
        ref = cr.boundary(name)
        assert not any(ref["frames"][f].any() for f in range(cr.B_ZERO)) and not ref["sched"][1]
        for c in cr.cases(ref):
            if c["frame"] >= cr.B_ZERO:
                continue
            assert c["meter"]["sum_sq"] == 0 and c["meter"]["clipped"] == 0 and not ref["want"][c["frame"]]["payload"][c["leaf"]].any()
            key = (c["cfg"].silent_ms, c["cfg"].lo_ms)
            kind = cr.kind_of(c)
            assert kind == {(0, 0): "window", (0, 1): "cold", (1, 1): "silent"}[key], c
            seen.add(kind)
            if kind == "cold":
                q = 2 if c["frame"] == 1 else 1
                assert c["cfg"].hold_frames == 1 and c["rec"]["quiet_run"] == q and c["rec"]["action"] == int(q > 1), c
            else:
                assert c["rec"]["quiet_run"] == 0, c
    assert seen == {"window", "cold", "silent"}


def test_clipped_alone_is_hot():
    """hi_ms = 2^30, exactly one wrapped sample, at an index past the first meter record: hot.  Next to it the same leaf at the
    gain one notch lower: nothing wraps, and the frame is in the window."""
    hot, calm = [], []
    for c in _boundary_cases():
        if c["frame"] in cr.B_CLIP and c["cfg"].hi_ms == cr.FULL and c["cfg"].lo_ms == 1 and c["meter"]["n_values"] > cr.TILE:
            if c["meter"]["clipped"] == 1:
                assert c["wrapped"][0] >= cr.TILE and c["meter"]["sum_sq"] <= cr.FULL * c["meter"]["n_values"]
                assert cr.kind_of(c) == "hot" and c["rec"]["action"] == -1
                hot.append((c["tree"], c["leaf"]))
            elif c["meter"]["clipped"] == 0:
                assert cr.kind_of(c) == "window" and c["rec"]["action"] == 0
                calm.append((c["tree"], c["leaf"]))
    print("clipped alone:", hot)
    assert len(hot) >= 3 and set(hot) <= set(calm) and {t for t, _ in hot} == set(cr.TREES)


def test_hold_frames():
    """Under one setting and no sdrx_set_agc in between: cold, cold, silent, cold, in-window, cold, hot, cold with
    hold_frames 0 (a raise in the first cold frame), 1 (in the second) and 2^32 - 1 (never); quiet_run counts 1, 2, 2, 3, 0, 1, 0, 1."""
    f0 = cr.B_ZERO + cr.B_CASE
    holds = {}
    for name in cr.TREES:
        ref = cr.boundary(name)
        assert ref["hold_leaves"]
        for f in range(f0 + 1, f0 + cr.B_HOLD):
            assert all(kind != "agc" for kind, _, _ in ref["sched"][f]), (name, f)
        by = {(c["leaf"], c["frame"]): c for c in cr.cases(ref)}
        for i in ref["hold_leaves"]:
            row = [by[(i, f)] for f in range(f0, f0 + cr.B_HOLD)]
            assert tuple(cr.kind_of(c) for c in row) == cr.HOLD_PATTERN, (name, i)
            assert tuple(c["rec"]["quiet_run"] for c in row) == cr.HOLD_QUIET, (name, i)
            hold = row[0]["cfg"].hold_frames
            want = {0: (1, 1, 0, 1, 0, 1, -1, 1), 1: (0, 1, 0, 1, 0, 0, -1, 0), cr.HOLD_MAX: (0, 0, 0, 0, 0, 0, -1, 0)}[hold]
            assert tuple(c["rec"]["action"] for c in row) == want, (name, i, hold)
            assert all(_bits(c["rec"]["gain_next"]) == _bits(c["g"]) for c in row), "the gain is frozen"
            holds[hold] = holds.get(hold, 0) + 1
    print("hold_frames -> leaves:", holds)
    assert set(holds) == {0, 1, cr.HOLD_MAX}


def _longest_free_run(rows, step) -> int:
    """The longest run of consecutive frames in which the gain moved by exactly one float32 multiply: action != 0 and
    gain_next == fl(g * step) != g -- no limit in the way"""
    best = run = 0
    for c in rows:
        g = np.float32(c["g"])
        with np.errstate(over="ignore"):
            x = g * np.float32(getattr(c["cfg"], step))
        ok = c["rec"]["action"] == (1 if step == "up" else -1) and _bits(c["rec"]["gain_next"]) == _bits(x) != _bits(g)
        run = run + 1 if ok else 0
        best = max(best, run)
    return best


def test_multiply_and_clamp_cases():
    """Every role of the schedule occurs and does what it is there for.  On the "free" leaves the gain compounds over at least
    six consecutive frames, each step one float32 multiply with no limit in reach -- raises and lowerings, on several leaves
    and on a leaf with several meter records; on the "compound" leaves it reaches a limit and stays there."""
    n = dict.fromkeys(("overflow", "above_max_down", "below_min_up", "outside_stays_above", "outside_stays_below", "pinned",
                       "reaches_ceiling", "reaches_floor", "free_up6", "free_down6", "free_up6_several_records", "free_down6_several_records"), 0)
    runs = {"up": [], "down": []}
    for name in cr.TREES:
        ref = cr.clamp(name)
        assert not any(ref["frames"][f].any() for f in range(cr.C_ZERO))
        by = {}
        for c in cr.cases(ref):
            by.setdefault(c["leaf"], []).append(c)
        for i, row in by.items():
            r0, r1 = ref["roles"][i]
            zero, loud = row[:cr.C_ZERO], row[cr.C_ZERO:]
            several = ref["topo"].vfos[i].n_out > cr.TILE
            assert len(zero) == cr.C_ZERO and len(loud) == cr.C_LOUD
            assert all(1.0 <= c["cfg"].up < 3.0 and 0.2 < c["cfg"].down <= 1.0 for c in row)
            for c in row:  # full mantissas: neither double is a float32, so a product taken in double rounds twice
                assert float(np.float32(c["cfg"].up)) != c["cfg"].up and float(np.float32(c["cfg"].down)) != c["cfg"].down, (name, i)
            assert all(_bits(b["g"]) == _bits(a["rec"]["gain_next"]) for a, b in zip(zero, zero[1:])), "the gain compounds"
            assert all(_bits(b["g"]) == _bits(a["rec"]["gain_next"]) for a, b in zip(loud, loud[1:]))
            with np.errstate(over="ignore"):
                if r0 == "overflow":
                    inf = [c for c in zero if np.isinf(np.float32(c["g"]) * np.float32(c["cfg"].up))]
                    assert inf and all(_bits(c["rec"]["gain_next"]) == _bits(cr.FLT_MAX) and c["rec"]["action"] == 1 for c in inf)
                    n["overflow"] += 1
            if r0 == "above_max_cold":
                c = zero[0]
                assert c["g"] > c["cfg"].gain_max and c["rec"]["action"] == 1 and _bits(c["rec"]["gain_next"]) == _bits(c["cfg"].gain_max)
                n["above_max_down"] += 1
            if r0 == "outside_window":
                for c in zero:
                    assert cr.kind_of(c) == "window" and c["rec"]["action"] == 0 and _bits(c["rec"]["gain_next"]) == _bits(zero[0]["g"])
                    assert not (c["cfg"].gain_min <= c["g"] <= c["cfg"].gain_max)
                n["outside_stays_above" if zero[0]["g"] > zero[0]["cfg"].gain_max else "outside_stays_below"] += 1
            if r0 == "pinned":
                assert zero[0]["cfg"].gain_min == zero[0]["cfg"].gain_max and all(_bits(c["rec"]["gain_next"]) == _bits(c["cfg"].gain_max) for c in zero)
                n["pinned"] += 1
            if r0 == "compound":
                assert all(c["rec"]["action"] == 1 for c in zero) and _longest_free_run(zero, "up") >= 3
                assert _bits(zero[-1]["rec"]["gain_next"]) == _bits(zero[-1]["cfg"].gain_max), "the ceiling was within reach"
                n["reaches_ceiling"] += 1
            if r0 == "free":
                k = _longest_free_run(zero, "up")
                runs["up"].append(k)
                assert k == cr.C_ZERO, (name, i, "seven raises, one multiply each", k)
                n["free_up6"] += k >= 6
                n["free_up6_several_records"] += k >= 6 and several
            if r1 == "below_min_hot" and cr.kind_of(loud[0]) == "hot":
                c = loud[0]
                assert c["g"] < c["cfg"].gain_min and c["rec"]["action"] == -1 and _bits(c["rec"]["gain_next"]) == _bits(c["cfg"].gain_min)
                n["below_min_up"] += 1
            if r1 == "compound":
                n["reaches_floor"] += any(c["rec"]["action"] == -1 and _bits(c["rec"]["gain_next"]) == _bits(c["cfg"].gain_min) for c in loud)
            if r1 == "free":
                k = _longest_free_run(loud, "down")
                runs["down"].append(k)
                n["free_down6"] += k >= 6
                n["free_down6_several_records"] += k >= 6 and several
    print("multiply and clamp:", n, "longest runs of free multiplies:", runs)
    assert all(v >= 1 for v in n.values()), n
    assert n["free_up6"] >= 3 and n["free_down6"] >= 3, n


def test_the_wide_tree():
    """520 USB leaves: three blocks of 256 with 8 in the last; settings that differ between neighbouring slots and between slot
    k and k +- 256 in every field; shuffled id lists of the seven sizes; every block sees every decision."""
    ref = cr.wide()
    slots = ref["slots"]
    assert len(slots) == cr.W_LEAVES >= 513 and list(slots) == sorted(slots) and cr.W_LEAVES % 256 == 8 and cr.W_LEAVES % 64 == 8
    fields = ("lo_ms", "hi_ms", "silent_ms", "hold_frames", "up", "down", "gain_min", "gain_max")
    for k in range(cr.W_LEAVES):
        for other in (k + 1, k + 256, k - 256):
            if 0 <= other < cr.W_LEAVES:
                a, b = cr.wide_cfg(k), cr.wide_cfg(other)
                assert all(_bits(getattr(a, f)) != _bits(getattr(b, f)) if isinstance(getattr(a, f), float) else getattr(a, f) != getattr(b, f)
                           for f in fields), (k, other)
        assert agc.invalid(cr.wide_cfg(k)) is None
    lists = [ids for calls in ref["sched"] for kind, ids, _ in calls if kind == "agc"]
    assert tuple(len(x) for x in lists) == cr.W_SIZES
    for ids in lists:
        assert len(set(ids)) == len(ids) and (len(ids) == 1 or list(ids) != sorted(ids))
    final = cr.settings_after(ref)[3][-1]
    slot_of = {i: k for k, i in enumerate(slots)}
    assert all(final[i] == cr.wide_cfg(slot_of[i]) for i in slots)
    gains = dict(zip(ref["sched"][3][-2][1], ref["sched"][3][-2][2]))
    assert all(_bits(gains[slots[k]]) != _bits(gains[slots[k + 1]]) for k in range(cr.W_LEAVES - 1))
    assert all(_bits(gains[slots[k]]) != _bits(gains[slots[k + 256]]) for k in range(cr.W_LEAVES - 256))
    # a leaf named before frame 1 alone has counted two cold frames in frame 2, one named again has counted one
    named1, named2 = set(lists[0]) | set(lists[1]) | set(lists[2]), set(lists[3]) | set(lists[4])
    q2 = {i: ref["want"][2]["agc"][i]["quiet_run"] for i in slots}
    assert {q2[i] for i in named1 - named2} == {2} and {q2[i] for i in named2} == {1} and {q2[i] for i in set(slots) - named1 - named2} == {0}
    assert named1 - named2 and named1 & named2
    seen = {}
    for c in cr.cases(ref):
        if c["frame"] >= 3:
            key = (slot_of[c["leaf"]] // 256, cr.kind_of(c), c["rec"]["action"])
            seen[key] = seen.get(key, 0) + 1
    print("wide tree (block, class, action) -> cases:", dict(sorted(seen.items())))
    for block in range(3):
        for kind, action in (("hot", -1), ("cold", 1), ("cold", 0), ("window", 0), ("silent", 0)):
            assert seen.get((block, kind, action), 0) >= 1, (block, kind, action)
    assert all(ref["frames"][f].any() for f in (3, 4, 5)) and not ref["frames"][6].any() and len(ref["frames"]) == 7
    assert not any(ref["sched"][f] for f in (4, 5, 6)), "four frames follow the last call"
    # cold over hold_frames for more than two frames under the slot's own setting: a raise that had to wait for the third
    waited = [i for i in slots if [ref["want"][f]["agc"][i]["quiet_run"] for f in (3, 4, 5)] == [1, 2, 3]
              and [ref["want"][f]["agc"][i]["action"] for f in (3, 4, 5)] == [0, 0, 1]]
    print("wide tree: leaves that raise in their third cold frame:", len(waited))
    assert len(waited) >= 3 and len({slot_of[i] // 256 for i in waited}) >= 2


def test_every_mutant_is_exposed():
    """Per wrong rule the number of scheduled (leaf, frame) pairs whose record differs: at least one each -- except the clamp
    taken as fmaxf(fminf(x, gain_max), gain_min), which differs from the rule only for a NaN product.  No call sequence
    produces one (sdrx_set_gains refuses gains that are not finite; the steps are finite), so it is shown on the rule alone."""
    counts = {m: cr.exposure(m) for m in cr.mutants()}
    print("mutant -> scheduled cases that expose it:", counts, "of", len(cr.all_cases()))
    for m, n in counts.items():
        if m in cr.UNREACHABLE:
            assert n == 0, (m, n)
        else:
            assert n >= 1, (m, counts)
    # where the unreachable one would show: a NaN product clamps to gain_min by the rule, to gain_max by the mutant ...
    cfg = agc.Cfg(1, 1, 0, 0, 2.0, 0.5, 0.25, 8.0)
    nan_case = dict(cfg=cfg, q=0, g=np.float32("nan"), meter={"sum_sq": 0, "n_values": 4, "clipped": 4}, head=None)
    assert cr.rule(nan_case)[0] == _bits(0.25) and cr.rule(nan_case, "clamp_max_of_min")[0] == _bits(8.0)
    # ... and for every other float pattern the two clamps agree whenever gain_min <= gain_max
    rng = np.random.default_rng(4)
    x = np.concatenate([rng.integers(0, 1 << 32, 200000, dtype=np.uint64).astype(np.uint32).view(np.float32),
                        np.array([np.inf, -np.inf, 0.0, -0.0, cr.FLT_MAX, 1e-45], np.float32)])
    x = x[~np.isnan(x)]
    lo = np.abs(rng.standard_normal(x.size)).astype(np.float32) + np.float32(1e-3)
    hi = lo * np.float32(1.0 + np.abs(rng.standard_normal(x.size)))
    hi[::7] = lo[::7]
    a, b = np.fmin(np.fmax(x, lo), hi), np.fmax(np.fmin(x, hi), lo)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
