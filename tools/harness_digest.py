"""sha256 of every array that every entry of the host mirror's harness returns (ov_plane_amd/hostlib.py: run_msckf_update,
run_initialize, run_updater in its four modes, run_propagate, run_zupt, run_state_maintenance, run_sequence, run_change_anchors,
feature_jacobian_rep, the two formatting entries, a ten-frame Session), one call per option on the scenes of tests/harness_calls.py.
Two checkouts whose harness computes the same bits print the same list; copy this file and tests/harness_calls.py into the other one:
    python tools/harness_digest.py --out this.json
    (cd ../other && python tools/harness_digest.py --out other.json)
    python tools/harness_digest.py --merge this.json ../other/other.json --out profiles/harness_refactor_digests.json"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def digest(out):
    h = hashlib.sha256()
    for k in sorted(out):
        a = np.ascontiguousarray(out[k])
        h.update(k.encode() + b"\0" + str(a.dtype).encode() + str(a.shape).encode() + b"\0" + a.tobytes())
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--merge", nargs=2, default=None, metavar=("THIS", "OTHER"))
    a = ap.parse_args()
    if a.merge:
        this, other = (json.load(open(p)) for p in a.merge)
        differ = sorted(k for k in set(this["digests"]) | set(other["digests"]) if this["digests"].get(k) != other["digests"].get(k))
        rec = dict(what="tools/harness_digest.py on this checkout and on a checkout of the commit in front of it, same machine, same visit",
                   this=this, other=other, differ=differ, equal=not differ)
        print("equal entry for entry:", rec["equal"], differ)
    else:
        from ov_plane_amd import hostlib
        from ov_plane_amd.build import build_host
        from tests import harness_calls

        build_host()
        # which harness this checkout has: options handed over per call (RunOpts), or armed through ovph_set_* before it
        rec = dict(options_per_call=hasattr(hostlib, "RunOpts"), digests={})
        for name, call in harness_calls.cases(hostlib):
            rec["digests"][name] = digest(harness_calls.flat(call()))
            print(name, rec["digests"][name], flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)
    if a.merge and not rec["equal"]:
        sys.exit(1)


if __name__ == "__main__":
    main()
