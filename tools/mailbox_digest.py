"""sha256 per entry point that returns its results through a pinned mailbox (csrc/ovp_mailbox.h), over the raw bytes of what the
C-ABI entry returns and the covariance afterwards: the calls of tests/mailbox_calls.py, one small fixed scene each, all on ONE
context in this order, then one detector frame.  Two builds of libovplane_hip.so that compute the same bits print the same list (the
second one selected with OVP_LIB_AB, as tools/plane_loop_digest.py does):
    python tools/mailbox_digest.py --out this.json
    OVP_LIB_AB=path/to/other/libovplane_hip.so python tools/mailbox_digest.py --out other.json
    python tools/mailbox_digest.py --merge this.json other.json --out profiles/mailbox_refactor_digests.json"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def digest(out):
    h = hashlib.sha256()
    for k in sorted(out):
        h.update(k.encode() + b"\0" + np.ascontiguousarray(out[k]).tobytes())
    return h.hexdigest()


def sites(capi):
    import mailbox_calls as mc

    ctx = mc.new_context(capi)
    for call in (mc.point_update, mc.point_update_async, mc.ekf_update, mc.ekf_update_info_form, mc.cov_initialize, mc.cov_propagate,
                 mc.slam_update, mc.slam_delayed_init, mc.plane_loop, mc.plane_loop_one):
        yield call.__name__, call(capi, ctx)
    ctx.close()
    history, frames = mc.detector_frames()
    ctx = capi.Context(64, 4, 8)
    det = capi.PlaneDetector(ctx)
    for fr in history:
        det.feed(*fr)
    yield "detector_frame", mc.detector_frame(det, frames[0])
    det.close()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--merge", nargs=2, default=None, metavar=("THIS", "OTHER"))
    a = ap.parse_args()
    if a.merge:
        this, other = (json.load(open(p)) for p in a.merge)
        rec = dict(what="tools/mailbox_digest.py with this checkout's library and with the build of the commit in front of it",
                   this=this, other=other, equal=this["digests"] == other["digests"])
        print("equal entry for entry:", rec["equal"])
    else:
        from ov_plane_amd import capi
        from ov_plane_amd.build import source_tree_hash

        rec = dict(library=os.path.relpath(capi.LIB_PATH, ROOT), source_tree_hash_of_this_checkout=source_tree_hash(), digests={})
        for name, out in sites(capi):
            rec["digests"][name] = digest(out)
            print(name, rec["digests"][name])
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)
    if a.merge and not rec["equal"]:
        sys.exit(1)


if __name__ == "__main__":
    main()
