"""CPU tests of the feature database's yardstick (tests/featdb_ref.py, tests/featdb_cases.py) and of the library's boundary: the new
symbols and struct layouts, the restatement against expectations written out by hand, the mutants - one recalled convention
changed at a time - and the C++ mirror's pure list logic (ov_plane_featdb_select.h) as a stand-alone sanitized program."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import featdb_cases  # noqa: E402
import featdb_ref  # noqa: E402
from featdb_cases import BIG, T  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["ovp_featdb_create", "ovp_featdb_destroy", "ovp_featdb_reset", "ovp_featdb_append", "ovp_featdb_classify_defaults",
           "ovp_featdb_classify", "ovp_featdb_mark_deleted", "ovp_featdb_gather", "ovp_featdb_triangulate", "ovp_featdb_cleanup",
           "ovp_featdb_get", "ovp_featdb_debug"]


def test_header_declares_and_library_exports_the_entries(hiplib):
    hdr = open(os.path.join(ROOT, "include", "ovplane_hip.h")).read()
    L = hiplib.lib()
    for s in SYMBOLS:
        assert re.search(r"\b%s\(" % s, hdr) and s in hiplib.EXPORTS and hasattr(L, s), s
    assert "int ovp_featdb_gather(ovp_ctx *ctx, int n, const int64_t *ids, const int *old_index, const double *clone_times, int n_clones);" in hdr
    assert "int ovp_featdb_cleanup(ovp_ctx *ctx, int do_cleanup, double measurements_before_or_nan);" in hdr
    for name, cls in (("ovp_featdb_classify_in", hiplib.FeatDbClassifyIn), ("ovp_featdb_classify_out", hiplib.FeatDbClassifyOut)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
        fields = []
        for decl in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";"):
            d = decl.strip()
            if d:
                fields.append(re.sub(r"\[\d+\]", "", d.split()[-1].lstrip("*")))
        assert fields == [f[0] for f in cls._fields_], (fields, cls._fields_)
    assert ctypes.sizeof(hiplib.FeatDbClassifyIn) == 40 and hiplib.FeatDbClassifyIn.t_now.offset == 16
    assert ctypes.sizeof(hiplib.FeatDbClassifyOut) == 64 and hiplib.FeatDbClassifyOut.totals.offset == 48
    a = hiplib.FeatDbClassifyIn()
    L.ovp_featdb_classify_defaults(ctypes.byref(a))
    assert (a.n_clones, a.max_clone_size, a.want_marg, a.t_now) == (0, 11, 1, 0.0)
    assert L.ovp_featdb_create(None, 4, 3) == -1 and L.ovp_featdb_cleanup(None, 1, 0.0) == -1   # OVP_E_ARG on a null context
    src = open(os.path.join(ROOT, "ov_plane_amd", "csrc", "k_featdb.hip")).read()
    for k in ("k_featdb_append", "k_featdb_classify", "k_featdb_gather", "k_featdb_cleanup"):
        assert "void %s(" % k in src


def _table(name, which=0):
    recs = [r for r in featdb_cases.reference(name) if r[0] == "classify"]
    r = recs[which]
    return dict(ids=np.frombuffer(r[1], np.int64), cls=np.frombuffer(r[2], np.int32), count=np.frombuffer(r[3], np.int32),
                cleaned=np.frombuffer(r[4], np.int32), flags=np.frombuffer(r[5], np.uint8), totals=np.frombuffer(r[6], np.int32))


def test_restatement_against_expectations_by_hand():
    t = _table("conventions")
    assert (t["ids"] - BIG).tolist() == [50, 51, 52, 53, 54, 55], "ascending id, whatever the append order"
    # 50: max_clone_size + 1 with the marginalisation time; 51: exactly max_clone_size, lost AND marg; 52: one ulp beside; 54: lost
    assert t["cls"].tolist() == [featdb_ref.MAXTRACK, featdb_ref.MARG, featdb_ref.NONE, featdb_ref.NONE, featdb_ref.LOST, featdb_ref.NONE]
    assert t["count"].tolist() == [4, 3, 3, 2, 1, 2] and t["cleaned"].tolist() == [4, 3, 2, 1, 0, 2]
    assert t["flags"].tolist() == [0, 0, 0, 1, 1, 0] and t["totals"].tolist() == [1, 1, 1, 0]
    off = _table("conventions", 1)          # want_marg false: nothing is marg, the lost ones stay lost
    assert off["cls"].tolist() == [0, featdb_ref.LOST, 0, 0, featdb_ref.LOST, 0]
    late = _table("conventions", 2)         # 51 and 54 are to_delete: skipped by both queries, 51 still collected T(5)
    assert late["cls"].tolist()[1] == featdb_ref.NONE and late["count"].tolist()[1] == 4 and late["flags"].tolist()[1] & featdb_ref.FLAG_DELETED
    rec = featdb_cases.reference("conventions")
    sel = [r for r in rec if r[0] == "select"]
    assert sel[0][1:] == ((BIG + 54,), (BIG + 51,), (), (BIG + 50,), (BIG + 55,), (BIG + 777,)), "the maxtrack becomes a new SLAM feature"
    assert sel[1][1:] == ((BIG + 54,), (BIG + 51,), (BIG + 50,), (), (BIG + 55,), (BIG + 777,)), "before the SLAM delay it stays a maxtrack"
    assert sel[2][1:] == ((BIG + 54,), (BIG + 51,), (BIG + 50,), (), (BIG + 55, BIG + 53), ()), "no room: max_slam_features landmarks"
    gat = [r for r in rec if r[0] == "gather"]
    assert [g[1] for g in gat] == [-1, -1, -6, 0, 0, 0, -1], "cleaned to nothing, unknown, no former batch, ..., an old index outside"
    assert gat[3][2:] == gat[4][2:], "the same list gathered twice"
    ci = np.frombuffer(gat[3][4], np.int32).reshape(4, 8)
    assert ci[0].tolist() == [0, 1, 2, 3, -1, -1, -1, -1] and ci[1].tolist() == [2, 3] + [-1] * 6 and ci[3].tolist() == [3] + [-1] * 7
    assert np.frombuffer(gat[3][5], np.int32).tolist() == [4, 2, 3, 1]
    uv = np.frombuffer(gat[3][2], np.float32).reshape(4, 8, 2)
    assert uv[1, 0].tobytes() == featdb_cases.obs([BIG + 52], 3)[0].tobytes() and not uv[1, 2:].any()
    cl = [np.frombuffer(r[1], np.int64).reshape(-1, 3) for r in rec if r[0] == "cleanup"]
    assert (cl[0] - [BIG, 0, 0]).tolist() == [[50, 5, 0], [51, 0, 1], [52, 3, 0], [53, 2, 0], [54, 0, 1], [55, 2, 0]]
    assert (cl[1] - [BIG, 0, 0]).tolist() == [[50, 2, 0], [52, 1, 0], [53, 1, 0], [55, 1, 0]], "the observation at the time stays"
    assert cl[2][:, 1:].tolist() == [[0, 1]] * 4, "every emptied slot is freed"


def test_small_table_by_hand():
    rec = featdb_cases.reference("s4_m3")
    assert [r[1] for r in rec if r[0] == "append"] == [0, 0, -2, 0, -2, 0, 0, 0, -2, 0]
    rb = [r for r in rec if r[0] == "readback"]
    assert rb[0] == rb[1] and rb[2] == rb[3], "a refused frame leaves the table as it was"
    t = _table("s4_m3")
    assert t["ids"].tolist() == [5, 7, 9, 12] and t["cls"].tolist() == [3, 0, 3, 2] and t["count"].tolist() == [3, 2, 3, 2]
    assert [f is None for f in rb[-1][1:]] == [True, True, True, True, False, False, False], "5, 7, 9, 12 have gone; 20, 21, 99 live"
    big = _table("m32")
    assert big["count"].tolist() == [32, 31, 30, 29, 28, 27, 26, 25] and big["cleaned"].tolist()[0] == 31 and big["cls"].tolist()[:3] == [3, 3, 0]
    assert 65 <= featdb_cases.case("s70_m8")[1] <= 70


@pytest.mark.parametrize("name", list(featdb_ref.MUTANTS))
def test_mutant_differs_on_a_case(name):
    caught = [c for c in featdb_cases.IDS if featdb_cases.reference(c, featdb_ref.mutant(name)) != featdb_cases.reference(c)]
    print("%s: differs on %s" % (name, caught))
    assert caught, "the mutant %s equals the restatement on every case" % name


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("featdb_host") / "featdb_host_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "ov_plane_amd", "csrc", "host"), "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "featdb_host_main.cpp"), "-o", exe])
    return exe


def test_list_logic_of_the_mirror_equals_select(host_exe, tmp_path, hiplib):
    """every (class table, select arguments) pair the cases meet, and a few tables of random classes: the sanitized C++ function,
    the restatement's select and capi.featdb_select give the same six lists"""
    probes = []
    for c in featdb_cases.IDS:
        table = None
        for op, r in zip(featdb_cases.case(c)[0], featdb_cases.reference(c)):
            if op[0] == "classify":
                table = (np.frombuffer(r[1], np.int64), np.frombuffer(r[2], np.int32))
            if op[0] == "select":
                probes.append(table + tuple(op[1:]))
    rng = np.random.default_rng(3)
    for n, nl, ms in ((0, 0, 3), (0, 2, 3), (40, 5, 9), (40, 5, 5), (7, 0, 2), (64, 6, 0)):
        ids = np.sort(rng.choice(np.arange(1, 200, dtype=np.int64) + BIG, n, replace=False))
        probes.append((ids, rng.integers(0, 4, n).astype(np.int32), [int(v) for v in rng.choice(np.arange(1, 200) + BIG, nl, replace=False)], ms, True))
    assert len(probes) > 20
    for k, (ids, cls, lms, ms, ok) in enumerate(probes):
        f = tmp_path / ("in%d.txt" % k)
        f.write_text("%d %d %d %d\n" % (len(ids), len(lms), ms, ok) + "".join("%d %d\n" % (i, c) for i, c in zip(ids, cls)) + " ".join(str(v) for v in lms) + "\n")
        run = subprocess.run([host_exe, str(f)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert run.returncode == 0, run.stdout
        got = [tuple(int(v) for v in line.split()[1:]) for line in run.stdout.strip("\n").split("\n")]
        want = featdb_ref.select(ids, cls, ids, lms, ms, ok)
        keys = ("lost", "marg", "maxtracks", "slam_delayed", "slam_update", "landmarks_marg")
        assert got == [tuple(want[key]) for key in keys], k
        py = hiplib.featdb_select(ids, cls, lms, ms, ok)
        assert [tuple(py[key]) for key in keys] == got, k


def test_harness_exports_the_sequence_entry_and_the_option():
    from ov_plane_amd import hostlib
    from ov_plane_amd.build import build_host

    L = ctypes.CDLL(build_host())
    assert hasattr(L, "ovph_run_featdb_sequence") and hostlib.carries_option("featdb")
    hdr = open(os.path.join(ROOT, "ov_plane_amd", "csrc", "host", "ov_plane_host.h")).read()
    assert "bool gpu_featdb = false;" in hdr, "off by default"
    assert hostlib.RunOpts().featdb == 0


def test_mirror_header_compiles_against_the_c_abi():
    """the C++ mirror over the C-ABI: compiled (not linked, not run - it needs a device)"""
    src = '#include "ov_plane_featdb.h"\nint probe(ovp_ctx* c) { ov_plane::FeatureDatabase d(c, 4, 3); ov_plane::FeatDbSelection s; ' \
          'return d.select({1.0}, 1.0, 11, {}, 0, true, s) + d.cleanup() + d.cleanup_measurements(1.0); }\n'
    run = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I" + os.path.join(ROOT, "ov_plane_amd", "csrc", "host"),
                          "-I" + os.path.join(ROOT, "include"), "-x", "c++", "-"], input=src, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout
