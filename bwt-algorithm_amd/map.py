#!/usr/bin/env python3
"""Batched read mapping over the MI355X-native FM index (bwtmi.map): SMEM seeds
chained on the device, one PAF row per chain:

    python map.py IN.fa QUERIES [-l MIN_LEN] [--both-strands] [--long] [--max-occ N] [--max-gap N]
                  [--bandwidth N] [--min-score N] [--min-anchors N] [--cigar] [--extend] [--select] -o OUT.paf

(bwtmi/map.py lists every option.)
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bwtmi.map import main  # noqa: E402

if __name__ == "__main__":
    sys.exit(main())
