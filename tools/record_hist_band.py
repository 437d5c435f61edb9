#!/usr/bin/env python3
"""Writes tests/golden/hist_band_*.npz, the expectation of tests/test_hip_hist_band.py, from the library in force (the one
FRANKENZ_HIP_LIB names, else the tree's): run it with a release build of the commit whose bits are to be kept.  Needs a GPU.
    FRANKENZ_HIP_LIB=/path/to/parent/libfrankenz_hip.so python3 tools/record_hist_band.py [OUTDIR]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)
import test_hip_hist_band as t          # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else t.GOLDEN
os.makedirs(out, exist_ok=True)
for name in t.CASES:
    pr = t.problem(name, 2 * 16 * t.engine().cu_count() + 37 if name == 'rounds' else None)      # (rounds: more than two rounds of the launch)
    t.check_list_length(pr)
    got = t.run(pr)
    path = os.path.join(out, os.path.basename(t.fixture_path(name)))
    np.savez_compressed(path, N=np.int64(len(pr['X'])), form=np.array(got['form']), lmap=got['lmap'][:t.N],
                        levid=got['levid'][:t.N], pdfs=got['pdfs'][t.KEEP])
    print('%-18s M=%d n=%d form=%s nan rows=%d size=%d B' % (name, len(pr['Y']), pr['n'], got['form'],
                                                           int(np.isnan(got['pdfs']).all(axis=1).sum()), os.path.getsize(path)), flush=True)
