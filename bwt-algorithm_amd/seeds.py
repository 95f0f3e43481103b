#!/usr/bin/env python3
"""Batched SMEM seeding of reads on both strands over the MI355X-native FM
index (bwtmi.seeds):

    python seeds.py IN.fa QUERIES [-l MIN_LEN] [--both-strands] [--max-occ N] [--max-positions N] -o OUT.tsv
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bwtmi.seeds import main  # noqa: E402

if __name__ == "__main__":
    sys.exit(main())
