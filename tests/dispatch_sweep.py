"""The argument sweeps of the host queries behind the strip-convolution dispatch (QUERIES: the five of the forward and
data-gradient families) and behind the 3x3 weight-gradient family (WGRAD_QUERIES), shared by
tests/golden/make_golden_dispatch.py (records the answers) and tests/test_host_logic.py (compares them).

A query's answers over its argument grid are kept run-length encoded in grid order (last argument fastest); the
same (values, counts) pair is stored once however many switch settings produce it.
"""
import ctypes
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

    def __init__(self, lib, switches=SWITCHES):
        self.lib, self.switches = lib, switches

    def __enter__(self):
        self.saved = {k: int(self.lib.fr_get_option(k.encode(), dflt)) for k, (dflt, _v) in self.switches.items()}
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


# ---- the 3x3 weight-gradient family (fr_conv_wgrad_strip): a second query set with a fixture of its own
STRIDES = (1, 2)
WGRAD_GRID = (BATCHES, CHANNELS, CHANNELS, WIDTHS, STRIDES)  # B, Cout, Cin, W = gradient width, stride
WGRAD_SWITCHES = {"FRHIP_WGRAD_ROLL": (1, (1, 0))}
_DUMMY_SLAB = ctypes.c_float()  # a non-null slab for the argument checks; no host query dereferences it


def wgrad_args(struct, B, cout, cin, W, stride):
    """FrWgradArgs (``struct``: the ctypes class) of the square 3x3 pad-1 problem with a W x W gradient."""
    a = struct()
    a.B, a.Cout, a.SC, a.stride, a.pad, a.KH, a.KW = B, cout, cin, stride, 1, 3, 3
    a.GH = a.GW = W
    a.SH = a.SW = W * stride
    a.ldg, a.lda, a.pro, a.nsplit = cout, cin, 0, 1
    a.slab = ctypes.addressof(_DUMMY_SLAB)
    return a


def _at_nsplit(query, nsplit):
    def ask(lib, a):
        a.nsplit = nsplit
        return getattr(lib, query)(ctypes.byref(a))
    return ask


# name -> ask(lib, args); every query sees the arguments of wgrad_args with its own nsplit
WGRAD_QUERIES = {
    "fr_conv_wgrad_strip_groups|wgs=128": lambda lib, a: lib.fr_conv_wgrad_strip_groups(ctypes.byref(a), 128),
    "fr_conv_wgrad_strip_groups|wgs=256": lambda lib, a: lib.fr_conv_wgrad_strip_groups(ctypes.byref(a), 256),
    "fr_conv_wgrad_strip_supported": lambda lib, a: lib.fr_conv_wgrad_strip_supported(a.Cout, a.SC, a.GW),
    "fr_conv_wgrad_strip_defers|nsplit=1": _at_nsplit("fr_conv_wgrad_strip_defers", 1),
}
WGRAD_QUERIES.update(("fr_conv_wgrad_strip_kernel|nsplit=%d" % n, _at_nsplit("fr_conv_wgrad_strip_kernel", n))
                     for n in (1, 8, 128, 256))


def wgrad_settings():
    for v in WGRAD_SWITCHES["FRHIP_WGRAD_ROLL"][1]:
        yield {"FRHIP_WGRAD_ROLL": v}


def wgrad_key(setting, query):
    return "FRHIP_WGRAD_ROLL=%d|%s" % (setting["FRHIP_WGRAD_ROLL"], query)


def wgrad_answers(lib, struct):
    """name -> the query's answers over WGRAD_GRID, in grid order, as int32 arrays (one pass over the grid)."""
    n = int(np.prod([len(g) for g in WGRAD_GRID]))
    out = {q: np.empty(n, dtype=np.int32) for q in WGRAD_QUERIES}
    for k, t in enumerate(itertools.product(*WGRAD_GRID)):
        a = wgrad_args(struct, *t)
        for q, ask in WGRAD_QUERIES.items():
            out[q][k] = ask(lib, a)
    return out


def wgrad_arguments(flat_index):
    """(B, Cout, Cin, W, stride) at a position of WGRAD_GRID."""
    idx = np.unravel_index(int(flat_index), [len(g) for g in WGRAD_GRID])
    return tuple(int(g[i]) for g, i in zip(WGRAD_GRID, idx))
