"""The argument sweep of the five host queries behind the strip-convolution dispatch, shared by
tests/golden/make_golden_dispatch.py (records the answers) and tests/test_host_logic.py (compares them).

A query's answers over its argument grid are kept run-length encoded in grid order (last argument fastest); the
same (values, counts) pair is stored once however many switch settings produce it.
"""
import itertools

import numpy as np

BATCHES = range(1, 521)
CHANNELS = (64, 96, 128, 256, 512)
WIDTHS = (7, 14, 20, 28, 56, 112)
EPILOGUES = range(9)
MODES = (0, 2)

# query -> argument grid (the order of the C prototype)
QUERIES = {
    "fr_conv3x3_strip_parts": (BATCHES, CHANNELS, CHANNELS, WIDTHS, EPILOGUES),
    "fr_conv3x3_strip_takes_frag": (BATCHES, CHANNELS, CHANNELS, WIDTHS),
    "fr_conv3x3_strip_serves_resbn": (BATCHES, CHANNELS, WIDTHS),
    "fr_conv3x3_s2_strip_parts": (BATCHES, CHANNELS, CHANNELS, WIDTHS, MODES),
    "fr_conv3x3_s2_strip_takes_frag": (BATCHES, CHANNELS, WIDTHS, MODES),
}

# switch -> (default of its first reader in the library, swept values)
SWITCHES = {
    "FRHIP_ROLL64": (1, (0, 1)),
    "FRHIP_S2_WS": (1, (0, 1)),
    "FRHIP_SPLIT_STRIPS": (0, (0, 1)),
    "FRHIP_ROLL_NSEG": (-1, (-1, 2)),     # the two test hooks move together: default, or two row segments forced
    "FRHIP_S2ROLL_NSEG": (-1, (-1, 2)),
}


def settings():
    """Every swept combination of the switches, as dicts name -> value."""
    for r, w, s, n in itertools.product((0, 1), (0, 1), (0, 1), (-1, 2)):
        yield {"FRHIP_ROLL64": r, "FRHIP_S2_WS": w, "FRHIP_SPLIT_STRIPS": s, "FRHIP_ROLL_NSEG": n,
               "FRHIP_S2ROLL_NSEG": n}


def setting_key(setting, query):
    return "%s|%s" % (",".join("%s=%d" % (k, setting[k]) for k in SWITCHES), query)


class Switches(object):
    """Sets the swept switches through fr_set_option and puts back what was there (the environment's value or the
    library's default) on exit."""

    def __init__(self, lib):
        self.lib = lib

    def __enter__(self):
        self.saved = {k: int(self.lib.fr_get_option(k.encode(), dflt)) for k, (dflt, _v) in SWITCHES.items()}
        return self

    def set(self, setting):
        for k, v in setting.items():
            self.lib.fr_set_option(k.encode(), int(v))

    def __exit__(self, *exc):
        self.set(self.saved)


def answers(lib, query):
    """The query's answers over its grid, in grid order, as an int32 array."""
    f = getattr(lib, query)
    return np.fromiter((f(*t) for t in itertools.product(*QUERIES[query])), dtype=np.int32)


def arguments(query, flat_index):
    """The argument tuple at a position of the query's grid."""
    grid = QUERIES[query]
    idx = np.unravel_index(int(flat_index), [len(g) for g in grid])
    return tuple(int(g[i]) for g, i in zip(grid, idx))


def rle(a):
    """(values, counts) of the runs of a 1-D array."""
    cut = np.flatnonzero(np.diff(a)) + 1
    starts = np.concatenate(([0], cut))
    return a[starts].astype(np.int32), np.diff(np.concatenate((starts, [len(a)]))).astype(np.int32)
