#!/usr/bin/env python3
"""Generate tests/golden/g17_dispatch.npz: what the five host queries behind the strip-convolution dispatch
(fr_conv3x3_strip_parts / _takes_frag / _serves_resbn, fr_conv3x3_s2_strip_parts / _takes_frag) answer over the sweep
of tests/dispatch_sweep.py, under every swept setting of the run-time switches.

The fixture pins the dispatch of ONE build of the library, so it is recorded from the build whose behaviour is to be
kept -- the commit before a change to the selection code -- and never from the tree under test:

    FRHIP_LIB=/path/to/libfrhip.so-of-the-parent-commit python tests/golden/make_golden_dispatch.py

(the queries are host arithmetic: no GPU needed).  Stored: run-length encoded answers, one (values, counts) pair per
distinct answer grid, and ``index``: "<switch setting>|<query>" -> the pair that holds it.

    FRHIP_LIB=... python tests/golden/make_golden_dispatch.py wgrad

records tests/golden/g26_wgrad_dispatch.npz instead: the queries of the 3x3 weight-gradient family
(dispatch_sweep.WGRAD_QUERIES: fr_conv_wgrad_strip_groups at 128 and 256 workgroups, _supported, _defers,
fr_conv_wgrad_strip_kernel at four group counts) over batch x channels x channels x width x stride, with
FRHIP_WGRAD_ROLL on and off, in the same format.  The commit before the family's tables were folded into select_wgrad had
neither fr_conv_wgrad_strip_groups nor fr_conv_wgrad_strip_kernel, so g26 was recorded from a scratch copy of that commit
with only these two functions appended to its conv_wgrad_strip.hip (never committed): _kernel as the argument check and
the two shape predicates of that commit's fr_conv_wgrad_strip, its fr_wgrad_roll_serves / fr_wgrad_s2roll_serves and its
switch statements over the width, returning an id where they launched; _groups as "does _kernel serve the shape" and then
a transcription of the fills / tiles / groups arithmetic of that commit's BackbonePlan._wgrad with its two dictionaries.
Before recording, the transcription was compared over the whole grid, at 128 and 256 workgroups, with that arithmetic
lifted verbatim from the commit's engine.py into a throw-away script: equal everywhere.
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


def main_wgrad():
    from frhip import _lib
    out, index = {}, {}
    with S.Switches(_lib.lib, S.WGRAD_SWITCHES) as sw:
        for setting in S.wgrad_settings():
            sw.set(setting)
            for query, got in S.wgrad_answers(_lib.lib, _lib.FrWgradArgs).items():
                vals, counts = S.rle(got)
                name = hashlib.sha1(vals.tobytes() + counts.tobytes()).hexdigest()[:12]
                out["v_" + name], out["c_" + name] = vals, counts
                index[S.wgrad_key(setting, query)] = name
    out["index"] = np.frombuffer(json.dumps(index, sort_keys=True).encode(), dtype=np.uint8)
    path = os.path.join(HERE, "g26_wgrad_dispatch.npz")
    np.savez_compressed(path, **out)
    print("%s: %d answer grids, %d distinct, %d bytes, recorded from %s"
          % (path, len(index), (len(out) - 1) // 2, os.path.getsize(path), _lib.LIB_PATH))


if __name__ == "__main__":
    main_wgrad() if sys.argv[1:] == ["wgrad"] else main()
