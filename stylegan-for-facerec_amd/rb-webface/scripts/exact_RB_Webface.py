"""RB-WebFace evaluation with the exact operating point at chosen FPRs (not in the reference).

    python rb-webface/scripts/exact_RB_Webface.py --data_path <WebFace images> --partition_path <pair lists> \\
        --model_ckpt_path <Backbone_....pth> --config_name configs/<config>.py [--thresholds LO HI N] --exact_fpr F [F ...]

``test_RB_Webface.py`` beside this file is the reference's driver and stays as it is.  This script accepts every argument of
that driver, RUNS its ``evaluate_model`` -- so the reference's lines come out as that driver prints them -- and, with
``--exact_fpr F [F ...]``, prints after them one block per group with, per F,

* the exact threshold: the score with at most floor(F * pairs) impostor pairs above it (``frhip.pairwise.thresholds_at_fmr``:
  a three-pass radix select over the pair scores -- no grid, no interpolation),
* the FMR achieved there, and TPR = 1 - FNMR at that threshold (one mode-1 tally, the reference's strict ``<``),

and then a warning whenever F lies outside the FMR values of the threshold grid: there the ``np.interp`` behind the
``TPR@FPR`` lines clamps, and the printed number is the value at the grid's end.  The embeddings and the grid's FMR values of
each group are taken from the driver's own ``group_rates`` call as it runs, so nothing is embedded twice.  DESIGN.md 7a.1.
"""
import argparse
import importlib.util
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("rb_webface_driver", os.path.join(_HERE, "test_RB_Webface.py"))
driver = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(driver)  # puts the product root on sys.path as well

from frhip.pairwise import thresholds_at_fmr  # noqa: E402


def exact_rates(pos_emb, neg_emb, fprs, n_names_per_grp=5):
    """Per requested FPR: (fpr, threshold, achieved FMR, TPR).  The threshold is the exact order statistic of the impostor
    scores (at most floor(fpr * pairs) of them lie above it), the TPR is 1 - FNMR at that threshold."""
    points = thresholds_at_fmr(driver._on_device(neg_emb), fprs)  # one normalisation, shared passes
    return [(float(f), float(t), fmr, 1 - driver.calc_FNMR(pos_emb, float(t), n_names_per_grp))
            for f, (t, fmr) in zip(fprs, points)]


def evaluate_model(*args, exact_fpr=None, **kwargs):
    """``test_RB_Webface.evaluate_model(*args, **kwargs)``, then the exact lines of every group.  Returns that function's two
    dictionaries and a third, group -> list of ``exact_rates`` tuples (empty without ``exact_fpr``)."""
    groups = []  # (pos_emb, neg_emb, FMR values of the grid, rows per person) of each group_rates call of the driver
    inner = driver.group_rates

    def listening(pos_emb, neg_emb, thresholds, n_names_per_grp=5):
        fmr, fnmr = inner(pos_emb, neg_emb, thresholds, n_names_per_grp)
        if exact_fpr:
            groups.append((pos_emb, neg_emb, fmr, n_names_per_grp))
        return fmr, fnmr

    driver.group_rates = listening
    try:
        tpr_at3, tpr_at4 = driver.evaluate_model(*args, **kwargs)
    finally:
        driver.group_rates = inner

    exact = dict()
    for grp, (pos_emb, neg_emb, fmr, n_names_per_grp) in zip(tpr_at3, groups):  # the driver's group order
        exact[grp] = exact_rates(pos_emb, neg_emb, exact_fpr, n_names_per_grp)
        print("Group ", grp)
        for f, t, fmr_at, tpr in exact[grp]:
            print("exact TPR@FPR=%g" % f, tpr, "threshold", t, "fmr", fmr_at)
        for f, _t, _fmr_at, _tpr in exact[grp]:
            if not fmr.min() <= f <= fmr.max():
                print("warning: FPR=%g lies outside the FMR range [%g, %g] of the threshold grid: np.interp clamps there, "
                      "and a TPR@FPR line of that FPR is the value at the grid's end (move the grid with --thresholds)"
                      % (f, fmr.min(), fmr.max()))
        print()
    return tpr_at3, tpr_at4, exact


if __name__ == "__main__":
    parser = argparse.ArgumentParser(description="RB-WebFace evaluation with the exact threshold, FMR and TPR at chosen FPRs.")
    parser.add_argument("--data_path", type=str, default="../", help="root folder of the WebFace images")
    parser.add_argument("--partition_path", type=str, default="../",
                        help="folder with the pos_/neg_pairs_samples_<Group>.txt lists")
    parser.add_argument("--model_ckpt_path", type=str, help="backbone checkpoint written by train.py (Backbone_*.pth)")
    parser.add_argument("--config_name", type=str, help="config file the checkpoint was trained with (backbone name, COMPUTE_DTYPE)")
    parser.add_argument("--cpu_batch_size", type=int, default=1000, help="accepted for compatibility; the tallies run on the GPU")
    parser.add_argument("--cpu_n_jobs", type=int, default=2, help="accepted for compatibility; the tallies run on the GPU")
    parser.add_argument("--gpu_batch_size", type=int, default=50, help="images per forward pass")
    parser.add_argument("--thresholds", type=float, nargs=3, metavar=("LO", "HI", "N"), default=None,
                        help="np.linspace(LO, HI, N) instead of the default 0.3 0.6 20")
    parser.add_argument("--exact_fpr", type=float, nargs="+", metavar="F", default=None,
                        help="print the exact threshold, achieved FMR and TPR at each of these FPRs (no grid, no interpolation)")
    args = parser.parse_args()
    thresholds = None if args.thresholds is None else np.linspace(args.thresholds[0], args.thresholds[1], int(args.thresholds[2]))
    evaluate_model(args.config_name, args.model_ckpt_path, args.data_path, args.partition_path,
                   cpu_batch_size=args.cpu_batch_size, cpu_n_jobs=args.cpu_n_jobs, gpu_batch_size=args.gpu_batch_size,
                   thresholds=thresholds, exact_fpr=args.exact_fpr)
