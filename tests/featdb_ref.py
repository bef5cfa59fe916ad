"""numpy / plain-Python restatement of the feature database the device holds (k_featdb.hip): ext ov_core::FeatureDatabase
(update_feature, features_not_containing_newer, features_containing, get_feature, cleanup, cleanup_measurements), the cleaning of
update/UpdaterMSCKF.cpp:74-100 and the selection of VioManager::do_feature_propagate_update (core/VioManager.cpp:373-506).

UNPINNED: ov_core is not in the reference tree.  The database's methods are recalled from their published form, not verified
against a file; each recalled convention is one flag of CONV so that someone with ov_core at hand can correct one line, and each
has a mutant - the convention changed, nothing else - that the tests show the comparison catches.  The call sites (the selection,
the ct_meas < 2 verdict, margtimestep) are pinned and cited line by line.  Everything here is a copy or an integer decision: the
device is held to it bit for bit.

The reference's database is a hash map; the order of every list is this project's own rule: ascending feature id."""
import numpy as np

NONE, LOST, MARG, MAXTRACK = 0, 1, 2, 3
FLAG_TOO_FEW, FLAG_DELETED = 1, 2
E_ARG, E_CAPACITY, E_STATE = -1, -2, -6

CONV = dict(
    newer_ge=True,          # features_not_containing_newer: "newer" is a last time stamp >= t, not > t
    skip_deleted=True,      # both queries are called with skip_deleted = true and leave out to_delete features
    containing_exact=True,  # features_containing compares doubles with ==
    clean_exact=True,       # clean_old_measurements keeps a measurement iff its time stamp == a clone time
    lost_marg_is_marg=True,  # :405-415 a lost feature that is also in feats_marg leaves feats_lost
    maxtrack_gt=True,       # :424 size > max_clone_size, not >=
    deleted_collects=True,  # update_feature appends to a feature whose to_delete is set
    older_lt=True,          # cleanup_measurements(t) drops time stamps < t, the one at t stays
    free_empty=True,        # cleanup_measurements erases a feature left without measurements
    min_meas_2=True,        # UpdaterMSCKF.cpp:94 ct_meas < 2
)
MUTANTS = {
    "newer_is_strictly_later": dict(newer_ge=False), "queries_keep_deleted": dict(skip_deleted=False),
    "containing_within_tolerance": dict(containing_exact=False), "cleaning_within_tolerance": dict(clean_exact=False),
    "lost_and_marg_stays_lost": dict(lost_marg_is_marg=False), "maxtrack_at_clone_size": dict(maxtrack_gt=False),
    "deleted_stops_collecting": dict(deleted_collects=False), "older_includes_equal": dict(older_lt=False),
    "empty_feature_stays": dict(free_empty=False), "too_few_below_three": dict(min_meas_2=False),
}
TOL = 1e-9  # what the two "within tolerance" mutants use


def mutant(name):
    return dict(CONV, **MUTANTS[name])


class Refused(Exception):
    def __init__(self, code):
        super().__init__("refused with %d" % code)
        self.code = code


class FeatureDatabase:
    """S slots of M observations.  feats: id -> dict(ts [list of float], uv / uvn [list of float32 pairs], to_delete)."""

    def __init__(self, S, M, conv=CONV):
        self.S, self.M, self.conv = S, M, conv
        self.reset()

    def reset(self):
        self.feats = {}
        self.batch = None

    # ---- update_feature, one frame at a time ------------------------------------------------------------------------------------
    def update_feature(self, t, ids, uv, uvn):
        ids = [int(i) for i in ids]
        uv = np.asarray(uv, dtype=np.float32).reshape(-1, 2)
        uvn = np.asarray(uvn, dtype=np.float32).reshape(-1, 2)
        if len(set(ids)) != len(ids):
            raise Refused(E_ARG)
        fresh = [i for i in ids if i not in self.feats]
        if any(len(self.feats[i]["ts"]) >= self.M for i in ids if i in self.feats) or len(self.feats) + len(fresh) > self.S:
            raise Refused(E_CAPACITY)
        for k, i in enumerate(ids):
            f = self.feats.setdefault(i, dict(ts=[], uv=[], uvn=[], to_delete=False))
            if f["to_delete"] and not self.conv["deleted_collects"]:
                continue
            f["ts"].append(float(t)), f["uv"].append(uv[k].copy()), f["uvn"].append(uvn[k].copy())

    def get_feature(self, fid):
        f = self.feats.get(int(fid))
        if f is None:
            return None
        n = len(f["ts"])
        return dict(count=n, to_delete=int(f["to_delete"]), ts=np.array(f["ts"], dtype=np.float64),
                    uv=np.array(f["uv"], dtype=np.float32).reshape(n, 2), uv_norm=np.array(f["uvn"], dtype=np.float32).reshape(n, 2))

    def mark_deleted(self, ids):
        ids = [int(i) for i in ids]
        if any(i not in self.feats for i in ids):
            raise Refused(E_ARG)
        for i in ids:
            self.feats[i]["to_delete"] = True

    # ---- the two queries and the cleaning's count -----------------------------------------------------------------------------
    def _same(self, a, b, exact):
        return a == b if exact else abs(a - b) < TOL

    def _cleaned(self, f, clone_times):
        return sum(1 for x in f["ts"] if any(self._same(x, c, self.conv["clean_exact"]) for c in clone_times))

    def classify(self, clone_times, t_now, marg_time, max_clone_size, want_marg):
        cv = self.conv
        ids = sorted(self.feats)
        cls, count, cleaned, flags = [], [], [], []
        for i in ids:
            f = self.feats[i]
            skip = f["to_delete"] and cv["skip_deleted"]
            last = f["ts"][-1] if f["ts"] else None
            newer = last is not None and (last >= t_now if cv["newer_ge"] else last > t_now)
            lost = not skip and not newer
            marg = bool(want_marg) and not skip and any(self._same(x, marg_time, cv["containing_exact"]) for x in f["ts"])
            if marg and lost and not cv["lost_marg_is_marg"]:
                marg = False
            if marg:
                big = len(f["ts"]) > max_clone_size if cv["maxtrack_gt"] else len(f["ts"]) >= max_clone_size
                c = MAXTRACK if big else MARG
            else:
                c = LOST if lost else NONE
            k = self._cleaned(f, clone_times)
            cls.append(c), count.append(len(f["ts"])), cleaned.append(k)
            flags.append((FLAG_TOO_FEW if k < (2 if cv["min_meas_2"] else 3) else 0) | (FLAG_DELETED if f["to_delete"] else 0))
        cls = np.array(cls, dtype=np.int32)
        tot = [int((cls == LOST).sum()), int((cls == MARG).sum()), int((cls == MAXTRACK).sum()), sum(1 for f in flags if f & FLAG_DELETED)]
        return dict(ids=np.array(ids, dtype=np.int64), cls=cls, count=np.array(count, dtype=np.int32),
                    cleaned=np.array(cleaned, dtype=np.int32), flags=np.array(flags, dtype=np.uint8), totals=np.array(tot, dtype=np.int32))

    def features_not_containing_newer(self, t):
        r = self.classify([], t, np.inf, 1 << 30, False)
        return [int(i) for i, c in zip(r["ids"], r["cls"]) if c == LOST]

    def features_containing(self, t):
        r = self.classify([], -np.inf, t, 1 << 30, True)
        return [int(i) for i, c in zip(r["ids"], r["cls"]) if c == MARG]

    # ---- the batch -------------------------------------------------------------------------------------------------------------
    def gather(self, ids, clone_times, old_index=None):
        ids = [int(i) for i in ids]
        clone_times = [float(c) for c in clone_times]
        if any(i not in self.feats for i in ids):
            raise Refused(E_ARG)
        if old_index is not None and self.batch is None:
            raise Refused(E_STATE)
        for k, i in enumerate(ids):
            n = self._cleaned(self.feats[i], clone_times)
            if n == 0 or n > self.M:
                raise Refused(E_ARG)
            if old_index is not None and not 0 <= old_index[k] < len(self.batch["n_meas"]):
                raise Refused(E_ARG)
        F, M = len(ids), self.M
        uv, uvn = np.zeros((F, M, 2), dtype=np.float32), np.zeros((F, M, 2), dtype=np.float32)
        ci, nm = np.full((F, M), -1, dtype=np.int32), np.zeros(F, dtype=np.int32)
        p = np.zeros((F, 3))
        for k, i in enumerate(ids):
            f, at = self.feats[i], 0
            for x, a, b in zip(f["ts"], f["uv"], f["uvn"]):
                hit = [j for j, c in enumerate(clone_times) if self._same(x, c, self.conv["clean_exact"])]
                if hit:
                    uv[k, at], uvn[k, at], ci[k, at] = a, b, hit[0]
                    at += 1
            nm[k] = at
            if old_index is not None:
                p[k] = self.batch["p_FinG"][old_index[k]]
        self.batch = dict(uv=uv, uv_norm=uvn, clone_idx=ci, n_meas=nm, p_FinG=p)

    def gathered(self):
        return self.batch

    # ---- cleanup() and cleanup_measurements(t): [id, new count, freed] per feature that was live -------------------------------
    def cleanup(self, do_cleanup, before=float("nan")):
        out = []
        by_time = before == before
        if not self.feats or (not do_cleanup and not by_time):
            return np.zeros((0, 3), dtype=np.int64)
        for i in sorted(self.feats):
            f = self.feats[i]
            freed = bool(do_cleanup and f["to_delete"])
            if not freed and by_time:
                keep = [k for k, x in enumerate(f["ts"]) if not (x < before if self.conv["older_lt"] else x <= before)]
                for key in ("ts", "uv", "uvn"):
                    f[key] = [f[key][k] for k in keep]
                freed = not f["ts"] and self.conv["free_empty"]
            out.append((i, 0 if freed else len(f["ts"]), int(freed)))
            if freed:
                del self.feats[i]
        return np.array(out, dtype=np.int64).reshape(-1, 3)

    def cleanup_measurements(self, t):
        return self.cleanup(False, t)


def select(ids, cls, live_ids, landmark_ids, max_slam_features, slam_delay_ok):
    """core/VioManager.cpp:373-506 on a published class table (ids ascending, cls) - one camera, no ArUco (curr_aruco_tags = 0).
    live_ids: what get_feature finds (every id of the table).  Returns the five lists and the landmarks to marginalise."""
    lost = [int(i) for i, c in zip(ids, cls) if c == LOST]
    marg = [int(i) for i, c in zip(ids, cls) if c == MARG]
    maxtracks = [int(i) for i, c in zip(ids, cls) if c == MAXTRACK]
    landmark_ids = [int(i) for i in landmark_ids]
    slam = []
    # :447-460 the last valid_amount of the maxtracks become new SLAM features
    if max_slam_features > 0 and slam_delay_ok and len(landmark_ids) < max_slam_features:
        valid = min(max_slam_features - len(landmark_ids), len(maxtracks))
        if valid > 0:
            slam += maxtracks[len(maxtracks) - valid:]
            del maxtracks[len(maxtracks) - valid:]
    # :466-480 a landmark the tracker still holds is updated, one it lost is marginalised
    live = set(int(i) for i in live_ids)
    landmarks_marg = []
    for lm in landmark_ids:
        if lm in live:
            slam.append(lm)
        else:
            landmarks_marg.append(lm)
    left = set(landmark_ids) - set(landmarks_marg)
    # :488-501
    return dict(lost=lost, marg=marg, maxtracks=maxtracks, slam_delayed=[i for i in slam if i not in left],
                slam_update=[i for i in slam if i in left], landmarks_marg=landmarks_marg)
