"""Channel counts that are no multiple of 16, and images of 2, 4 and 5 channels: the REFERENCE'S OWN graph code (over
tests/golden/tf_standin.py) on tables such as [8, 12, 20] / [24, 40] / [10] and [4, 6] / [7] -- widths that
make_ref_graph_golden.py, fuzz_ref_graph.py and rect_ref_graph.py (multiples of 16 on 1- and 3-channel images throughout)
never ran.  Same vectors as rect_ref_graph.py: the forward values in both modes and the digest of every variable after
one training step.

The two sides cannot share a process (both packages are called `lib`):

    python tests/golden/chan_ref_graph.py --emit out.npz       # REFERENCE side (build container only)
    tests/test_conv_ch_cpu.py                                   # oracle side, against chan_ref_graph_golden.npz

FIXTURE TOOLING.  Nothing here is on the product path; only the --emit child reads the reference tree.  Its results are
stored in chan_ref_graph_golden.npz:

    python tests/golden/chan_ref_graph.py --emit tests/golden/chan_ref_graph_golden.npz
"""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import rect_ref_graph as R

REF = R.REF
ODD = [[8, 12, 20], [8, 12, 20], [24, 40], [24, 40], [10], [10]]      # 16x16 -> 16, 8, 4
NARROW = [[4, 6], [4, 6], [7]]                                        # 8x8 -> 8, 4

CASES = {
    'ac_odd': dict(ctor='ac_chain', hypers=dict(k_cpt=1.6e-8), tau=0.7, n=3, shape=(16, 16, 2), arch=ODD, seed=41),
    'cr_odd': dict(ctor='cr_chain', hypers=dict(k_cpt=4e-9), tau=0.9, n=3, shape=(16, 16, 4), arch=ODD, seed=42),
    'sr_narrow': dict(ctor='sr_chain', args=(3,), hypers={}, tau=None, n=3, shape=(8, 8, 5), arch=NARROW, seed=43),
}

build, case_inputs = R.build, R.case_inputs


def emit(path):
    """rect_ref_graph.emit over this module's cases (it walks its module's CASES)."""
    saved = R.CASES
    try:
        R.CASES = CASES
        R.emit(path)
    finally:
        R.CASES = saved


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--emit', required=True)
    emit(ap.parse_args().emit)
