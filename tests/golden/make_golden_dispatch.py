#!/usr/bin/env python3
"""Generate tests/golden/g17_dispatch.npz: what the five host queries behind the strip-convolution dispatch
(fr_conv3x3_strip_parts / _takes_frag / _serves_resbn, fr_conv3x3_s2_strip_parts / _takes_frag) answer over the sweep
of tests/dispatch_sweep.py, under every swept setting of the run-time switches.

The fixture pins the dispatch of ONE build of the library, so it is recorded from the build whose behaviour is to be
kept -- the commit before a change to the selection code -- and never from the tree under test:

    FRHIP_LIB=/path/to/libfrhip.so-of-the-parent-commit python tests/golden/make_golden_dispatch.py

(the queries are host arithmetic: no GPU needed).  Stored: run-length encoded answers, one (values, counts) pair per
distinct answer grid, and ``index``: "<switch setting>|<query>" -> the pair that holds it.
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "stylegan-for-facerec_amd"))
import dispatch_sweep as S  # noqa: E402


def main():
    from frhip import _lib
    out, index = {}, {}
    with S.Switches(_lib.lib) as sw:
        for setting in S.settings():
            sw.set(setting)
            for query in S.QUERIES:
                vals, counts = S.rle(S.answers(_lib.lib, query))
                name = hashlib.sha1(vals.tobytes() + counts.tobytes()).hexdigest()[:12]
                out["v_" + name], out["c_" + name] = vals, counts
                index[S.setting_key(setting, query)] = name
    out["index"] = np.frombuffer(json.dumps(index, sort_keys=True).encode(), dtype=np.uint8)
    path = os.path.join(HERE, "g17_dispatch.npz")
    np.savez_compressed(path, **out)
    print("%s: %d answer grids, %d distinct, %d bytes, recorded from %s"
          % (path, len(index), (len(out) - 1) // 2, os.path.getsize(path), _lib.LIB_PATH))


if __name__ == "__main__":
    main()
