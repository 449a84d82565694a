"""Shared inputs of test_dropout_host.py and test_gpu_dropout.py: the batch layouts of the counter-based Dropout tests.

OFFSETS is the ragged batch of the small cases: four videos of 1, 23, 2 and 7 rows - a one-row video first, a video of
several rows, and 33 rows in all, which is no multiple of anything the launch uses.  large_offsets() is the large
case: 300 videos of 1 .. 39 rows at LARGE_COLS = 512 columns, which has more (row, column quad) items than one trip of
the capped grid-stride launch covers (test_dropout_host.py checks that against the header's launch constants), so some
threads take a second item, and whose binary search over 301 offsets runs nine levels deep."""
import numpy as np

OFFSETS = [0, 1, 24, 26, 33]
SAMPLE_TABLE = [7, 2 ** 32 + 3, 0, 7]      # video 0 and video 3 share an id; video 1's id needs the high word
SMALL_COLS = 32
BUFFER_COLS = 40                            # the small masks are written into columns 4 .. 36 of a 40-wide buffer
BUFFER_ROWS = 37                            # ... and rows 0 .. 33 of 37
SENTINEL = -7.0

LARGE_VIDEOS = 300
LARGE_COLS = 512


def large_offsets():
    lengths = 1 + (np.arange(LARGE_VIDEOS, dtype=np.int64) * 7) % 39
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
