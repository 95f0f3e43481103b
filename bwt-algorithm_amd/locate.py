#!/usr/bin/env python3
"""Batched locate with mismatches on both strands over the MI355X-native FM
index (bwtmi.locate):

    python locate.py IN.fa PATTERNS [-k K] [--both-strands] [--max-candidates N] -o OUT.bed
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bwtmi.locate import main  # noqa: E402

if __name__ == "__main__":
    sys.exit(main())
