"""Scripted sequences for the feature database (tests/featdb_ref.py is the yardstick, k_featdb.hip the code under test): each case is
a list of operations that run(ops, db, select) applies to any object with the restatement's surface - featdb_ref.FeatureDatabase
under any convention, or capi.FeatureDatabase on the device - and turns into a list of records of plain bytes and integers.  Two
backends agree when their record lists are equal.  The shapes are the smallest at which the kernels can still go wrong."""
import numpy as np

import featdb_ref

BIG = 1 << 33   # ids above 2^32


def T(k):
    return 1000.0 + 0.05 * k   # (no multiple of 0.05 is a double: the clone times are arbitrary bit patterns)


def obs(ids, k):
    """what the tracker would hand over for feature `ids` in frame k: a pure function of (id, frame)"""
    i = np.asarray(ids, dtype=np.int64)
    uv = np.stack([(i % 997) + 0.25 * k, (i % 13) * 3.0 + 0.5 * k], axis=1).astype(np.float32).reshape(-1, 2)
    return uv, (uv * np.float32(0.001) - np.float32(0.3)).astype(np.float32)


def _code(fn, *a):
    try:
        fn(*a)
        return 0
    except Exception as e:   # featdb_ref.Refused or capi.OvpError: both carry .code
        return int(e.code)


def _feat_bytes(f):
    if f is None:
        return None
    return (int(f["count"]), int(f["to_delete"]), np.asarray(f["ts"], dtype=np.float64).tobytes(), np.asarray(f["uv"], dtype=np.float32).tobytes(),
            np.asarray(f["uv_norm"], dtype=np.float32).tobytes())


def run(ops, db, select):
    rec, table = [], None
    for op in ops:
        kind = op[0]
        if kind == "append":
            _, t, ids, k = op
            uv, uvn = obs(ids, k)
            rec.append(("append", _code(db.update_feature, t, ids, uv, uvn)))
        elif kind == "classify":
            table = db.classify(*op[1:])
            rec.append(("classify",) + tuple(np.asarray(table[key]).tobytes() for key in ("ids", "cls", "count", "cleaned", "flags", "totals")))
        elif kind == "select":
            s = select(table["ids"], table["cls"], *op[1:])
            rec.append(("select",) + tuple(tuple(s[key]) for key in ("lost", "marg", "maxtracks", "slam_delayed", "slam_update", "landmarks_marg")))
        elif kind == "queries":
            rec.append(("queries", tuple(db.features_not_containing_newer(op[1])), tuple(db.features_containing(op[1]))))
        elif kind == "mark":
            rec.append(("mark", _code(db.mark_deleted, op[1])))
        elif kind == "gather":
            code = _code(db.gather, *op[1:])
            g = db.gathered()
            rec.append(("gather", code) + (() if g is None else tuple(np.asarray(g[key]).tobytes() for key in ("uv", "uv_norm", "clone_idx", "n_meas", "p_FinG"))))
        elif kind == "cleanup":
            rec.append(("cleanup", np.asarray(db.cleanup(*op[1:]), dtype=np.int64).tobytes()))
        elif kind == "readback":
            rec.append(("readback",) + tuple(_feat_bytes(db.get_feature(i)) for i in op[1]))
        else:
            raise ValueError(kind)
    return rec


def _select_ref(ids, cls, *a):
    return featdb_ref.select(ids, cls, ids, *a)


# ---- the frame loop of core/VioManager.cpp:373-506, :855-869 as a generator of operations --------------------------------------
def frame_loop(S, M, W, frames, tracks, landmarks=(), max_slam=0):
    """tracks: id -> (first, last) frame.  Per frame: the frame's observations (descending id: unsorted on purpose), the class table
    over the clones after cloning (the last W + 1 frames), the selection, the batch of what was selected and can be stacked, to_delete
    on everything selected, cleanup() and - once the window is full - cleanup_measurements(margtimestep), a full read-back.  The
    lists come from the restatement under CONV; the operations are then fixed, whatever runs them."""
    db = featdb_ref.FeatureDatabase(S, M)
    ops, seen, peak = [], set(), 0
    for k in range(frames):
        ids = sorted((i for i, (a, b) in tracks.items() if a <= k <= b), reverse=True)
        seen |= set(ids)
        ct = [T(j) for j in range(max(0, k - W), k + 1)]
        want = len(ct) > W or len(ct) > 5
        head = [("append", T(k), ids, k), ("classify", ct, T(k), ct[0], W, want), ("select", list(landmarks), max_slam, True)]
        run(head[:1], db, _select_ref)
        peak = max(peak, len(db.feats))
        t = db.classify(ct, T(k), ct[0], W, want)
        s = featdb_ref.select(t["ids"], t["cls"], t["ids"], list(landmarks), max_slam, True)
        chosen = s["lost"] + s["marg"] + s["maxtracks"] + s["slam_delayed"] + s["slam_update"]
        enough = {int(i) for i, c in zip(t["ids"], t["cleaned"]) if c >= 2}
        rest = [("gather", [i for i in chosen if i in enough], ct, None), ("mark", chosen),
                ("cleanup", True, ct[0] if len(ct) > W else float("nan")), ("readback", sorted(seen))]
        run(rest, db, _select_ref)
        ops += head + rest
    return ops, peak


def s4_m3():
    """S = 4, M = 3, a 3-clone window, 6 frames: slot reuse after cleanup, a slot filled to exactly M, both capacity refusals with
    the table unchanged behind them, an empty frame, an empty gather"""
    every = [5, 7, 9, 12, 20, 21, 99]
    c3 = [T(0), T(1), T(2)]
    return [
        ("append", T(0), [12, 5, 9], 0), ("append", T(1), [5, 12, 9, 7], 1), ("readback", every),
        ("append", T(1) + 0.01, [99], 1), ("readback", every),                       # a fifth feature: refused, nothing touched
        ("append", T(2), [5, 9, 7], 2), ("readback", every),                         # 5 and 9 hold exactly M
        ("classify", c3, T(2), T(0), 2, True), ("select", [], 0, True),              # 12 is lost AND holds the marginalisation time
        ("append", T(3), [7, 5], 3), ("readback", every),                            # 5 is full: refused, 7 untouched too
        ("append", T(3), [], 3), ("gather", [], c3, None),
        ("gather", [5, 9, 12], c3, None), ("mark", [5, 12]),
        ("append", T(3), [12, 7], 3), ("classify", [T(1), T(2), T(3)], T(3), T(1), 2, True), ("queries", T(3)),
        ("cleanup", True, float("nan")), ("readback", every),
        ("append", T(4), [21, 20], 4), ("readback", every),                          # the freed slots are taken again
        ("append", T(4) + 0.01, [99], 4),                                            # and the table is full again
        ("cleanup", False, T(4)), ("readback", every),                               # 9 and 7 are emptied and go
        ("append", T(5), [20, 99], 5), ("readback", every),
    ]


def s70_m8():
    """S = 70, M = 8, window 6, 12 frames, 65 features live at once: more than one wave of slots, the last one partial; the second
    generation's ids lie above 2^32"""
    tracks = {1000 + i: (0, 1 + i % 11) for i in range(65)}
    tracks.update({BIG + 7 * j: (6 + j % 3, 6 + j % 3 + j % 5) for j in range(40)})
    return frame_loop(70, 8, 5, 12, tracks, landmarks=[1003, 1010, BIG + 14], max_slam=6)


def m32():
    """M = 32 and a window of 31 clones, 8 features: the pitch limit, a feature with 32 observations, the refusal of a 33rd"""
    ids = list(range(1, 9))
    ops = []
    for k in range(32):
        ops.append(("append", T(k), [i for i in reversed(ids) if i - 1 <= k], k))
    ct = [T(j) for j in range(1, 32)]
    ops += [("readback", ids), ("classify", ct, T(31), T(1), 30, True), ("select", [], 0, True), ("gather", ids, ct, None),
            ("gather", [8, 1, 3], ct, [7, 0, 2]),
            ("append", T(32), ids, 32), ("readback", ids),                           # feature 1 would hold 33: the frame is refused
            ("cleanup", False, T(1)), ("append", T(32), ids, 32), ("readback", ids),  # T(0) has gone: 31 + 1
            ("classify", [T(j) for j in range(2, 33)], T(32), T(2), 30, True), ("gather", ids, [T(j) for j in range(2, 33)], None)]
    return ops


def conventions():
    """one feature per recalled convention, ids above 2^32, appended out of order"""
    B = BIG
    t1b = float(np.nextafter(T(1), np.inf))   # one ulp beside a clone time
    every = [B + i for i in (50, 51, 52, 53, 54, 55, 777)]
    c4 = [T(1), T(2), T(3), T(4)]
    return [
        ("append", T(0), [B + 54, B + 53], 0), ("append", T(1), [B + 51, B + 50], 1), ("append", t1b, [B + 52], 1),
        ("append", T(2), [B + 50, B + 51], 2), ("append", T(3), [B + 55, B + 52, B + 51, B + 50], 3),
        ("append", T(4), [B + 53, B + 50, B + 52, B + 55], 4), ("readback", every),
        # 50: max_clone_size + 1 observations with the marginalisation time: maxtrack; 51: exactly max_clone_size, lost in this frame
        # and at the marginalisation time: marg; 52: one ulp beside it: nothing, and that observation is cleaned away; 53: cleaned
        # down to one; 54: lost, cleaned down to none
        ("classify", c4, T(4), T(1), 3, True), ("select", [B + 55, B + 777], 3, True), ("select", [B + 55, B + 777], 3, False),
        ("select", [B + 55, B + 53], 2, True),
        ("classify", c4, T(4), T(1), 3, False), ("select", [], 2, True),             # want_marg false
        ("queries", T(4)), ("queries", T(1)), ("queries", t1b),
        ("gather", [B + 54], c4, None), ("gather", [B + 9999], c4, None),            # nothing to stack; unknown: both refused
        ("gather", [B + 50, B + 52, B + 51, B + 53], c4, [0, 1, 2, 3]),              # no former batch
        ("gather", [B + 50, B + 52, B + 51, B + 53], c4, None), ("gather", [B + 50, B + 52, B + 51, B + 53], c4, None),
        ("gather", [B + 53, B + 50], c4, [3, 0]), ("gather", [B + 53], c4, [2]),      # the second: index 2 of a batch of two
        ("mark", [B + 9999]), ("mark", [B + 51, B + 54]),
        ("append", T(5), [B + 51, B + 50], 5), ("readback", every),                  # a deleted feature keeps collecting
        ("classify", [T(2), T(3), T(4), T(5)], T(5), T(2), 3, True), ("queries", T(5)), ("queries", T(2)),
        ("cleanup", True, float("nan")), ("readback", every),
        ("cleanup", False, T(4)), ("readback", every),                               # the observation AT the time stays
        ("cleanup", False, T(5) + 1.0), ("readback", every),                         # every slot emptied
        ("append", T(6), [B + 50], 6), ("classify", [T(6)], T(6), T(6), 3, False), ("readback", every),
    ]


_CACHE = {}


def case(name):
    """(operations, peak live features or None)"""
    if name not in _CACHE:
        r = CASES[name]()
        _CACHE[name] = r if isinstance(r, tuple) else (r, None)
    return _CACHE[name]


def dims(name):
    return {"s4_m3": (4, 3), "s70_m8": (70, 8), "m32": (8, 32), "conventions": (8, 8)}[name]


CASES = {"s4_m3": s4_m3, "s70_m8": s70_m8, "m32": m32, "conventions": conventions}
IDS = list(CASES)
_REF = {}


def reference(name, conv=featdb_ref.CONV):
    """the restatement's records: computed once per convention set and shared"""
    key = (name, tuple(sorted(conv.items())))
    if key not in _REF:
        S, M = dims(name)
        _REF[key] = run(case(name)[0], featdb_ref.FeatureDatabase(S, M, conv), _select_ref)
    return _REF[key]
