"""Pages whose block counts walk around the scan group of the page-box kernels (csrc/page_boxes.h: a word tests four table rows
at a time, the table is padded to whole groups): the inputs of one test each in tests/test_gpu_block_vote.py and
tests/test_gpu_block_scores.py; tests/test_blocks_ref_cpu.py asserts on the CPU that the oracle's answer for them is not empty.

Page k of 9 has B = k + 1 blocks -- 1 .. 9: every residue of the group of four twice, both sides of 4 and of 8 -- and 70 words,
more than one wave.  Block j is the cell [10 j, 0, 10 j + 5, 5]; word i lies inside cell i mod (B + 1), where the index B means
far away from every block.  ``nan_last``: the LAST block of every page has one NaN corner, so its words go to no block -- and a
padding row, which follows it in the table, must never be hit."""
import numpy as np

PAGES, WORDS = 9, 70
FAR = 100000


def scan_group_pages(nan_last=False):
    """[(word boxes int32 [70, 4], categories int32 [70], blocks float64 [B, 4])] for B = 1 .. 9."""
    pages = []
    for k in range(PAGES):
        n_blocks = k + 1
        blocks = np.asarray([[10.0 * j, 0.0, 10.0 * j + 5.0, 5.0] for j in range(n_blocks)], dtype=np.float64)
        if nan_last:
            blocks[-1, (k % 4)] = np.nan
        cell = np.arange(WORDS) % (n_blocks + 1)
        x0 = np.where(cell < n_blocks, 10 * cell + 1, FAR)
        words = np.stack([x0, np.full(WORDS, 1), x0 + 2, np.full(WORDS, 3)], axis=1).astype(np.int32)
        cats = ((7 * np.arange(WORDS) + k) % 13).astype(np.int32)
        pages.append((words, cats, blocks))
    return pages


def word_cells(k):
    """The cell of every word of page k: the page-local block the word lies in, or B = k + 1 for the far-away words."""
    return np.arange(WORDS) % (k + 2)
