#!/usr/bin/env python3
"""Derives tests/golden/shipped_nnet_conf.json: the text of every egs/*/*/nnet_conf/*.json of the reference checkout (voxceleb,
sre, fisher recipes; 81 single-task + 10 multitask configs), keyed by its path under the checkout.  The files hold settings only;
the text is kept byte for byte so that tests/test_host_io.py parses exactly what the reference ships, without the checkout.

Usage:  python tests/golden/make_shipped_nnet_conf.py <reference checkout>"""
import glob
import json
import os
import sys


def main(ref):
    files = sorted(glob.glob(os.path.join(ref, "egs", "*", "*", "nnet_conf", "*.json")))
    assert len(files) >= 90, "%d configs under %s" % (len(files), ref)
    out = {}
    for f in files:
        with open(f) as fh:
            out[os.path.relpath(f, ref)] = fh.read()
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "shipped_nnet_conf.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("%d configs -> %s" % (len(out), path))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__.rsplit("\n", 1)[-1])
    main(sys.argv[1])
