"""CPU reference of the block vote (gte_block_vote of include/gte.h, postprocessing.block_vote), written from its definition; plain Python /
numpy (it also runs where the GPU tests run), and a maker of layout blocks for synthetic pages.

The rule restates the words x blocks loop of the reference's get_objects_bboxs (postprocessing_2.py:240-258);
tests/golden/blocks_cases.json (tools/make_blocks_golden.py: the reference's own statements on generated pages) pins this
restatement to it:
  1. a word belongs to the FIRST block of its page (lowest index) whose rectangle meets the word's;
  2. both rectangles are normalised per axis (min / max of the two corners); the test is closed (touching counts), in float64;
     a block with a NaN coordinate meets nothing;
  3. the word adds 2 to the block's counter of its category if that is ``double_cat``, else 1; a category outside [0, n_cat)
     casts no vote (the word is still assigned);
  4. a block's label is the lowest category with the largest count, 0 for a block without votes."""
import numpy as np


def meets(word, block):
    """Rule 2 for one word (ints) and one block (floats, already divided by the scale factor)."""
    if any(v != v for v in block):
        return False
    left, top = max(min(word[0], word[2]), min(block[0], block[2])), max(min(word[1], word[3]), min(block[1], block[3]))
    right, bottom = min(max(word[0], word[2]), max(block[0], block[2])), min(max(word[1], word[3]), max(block[1], block[3]))
    return left <= right and top <= bottom


def vote_page(bboxs, cats, scaled_blocks, n_cat=13, double_cat=2):
    """One page -> (word_block [n] page-local or -1, votes [blocks][n_cat], labels [blocks]) as Python lists."""
    words = [[int(v) for v in w] for w in np.asarray(bboxs).reshape(-1, 4).tolist()]
    blocks = [[float(v) for v in b] for b in np.asarray(scaled_blocks, dtype=np.float64).reshape(-1, 4).tolist()]
    votes = [[0] * n_cat for _ in blocks]
    word_block = []
    for w, c in zip(words, [int(c) for c in cats]):
        hit = next((j for j, b in enumerate(blocks) if meets(w, b)), -1)
        word_block.append(hit)
        if hit >= 0 and 0 <= c < n_cat:
            votes[hit][c] += 2 if c == double_cat else 1
    return word_block, votes, [v.index(max(v)) for v in votes]


def vote_batch(bbox, node_off, word_cat, block_box, block_off, n_cat=13, double_cat=2):
    """The ABI's outputs for a batch: (word_block int32 [n] GLOBAL or -1, votes int32 [B, n_cat], label int32 [B])."""
    bbox, block_box = np.asarray(bbox).reshape(-1, 4), np.asarray(block_box, dtype=np.float64).reshape(-1, 4)
    word_block = np.full(bbox.shape[0], -1, dtype=np.int32)
    votes = np.zeros((block_box.shape[0], n_cat), dtype=np.int32)
    label = np.zeros(block_box.shape[0], dtype=np.int32)
    for p in range(len(node_off) - 1):
        n0, n1, b0, b1 = int(node_off[p]), int(node_off[p + 1]), int(block_off[p]), int(block_off[p + 1])
        wb, v, l = vote_page(bbox[n0:n1], np.asarray(word_cat)[n0:n1], block_box[b0:b1], n_cat, double_cat)
        word_block[n0:n1] = [b0 + j if j >= 0 else -1 for j in wb]
        votes[b0:b1] = np.asarray(v, dtype=np.int32).reshape(-1, n_cat)
        label[b0:b1] = l
    return word_block, votes, label


def synthetic_blocks(bboxs, rng, scale=0.36, cell=(260, 170), outside=0.05):
    """Layout blocks (PDF points: pixels x ``scale``) for a synthetic page: the words, but for a share ``outside`` of them, are
    binned into grid cells of ``cell`` pixels by their centre; every occupied cell gives one block, the union of its words' boxes,
    in a shuffled order.  Blocks of neighbouring cells may overlap (a word may meet two: the lower index takes it) and a word
    left out may still lie inside a block or outside all of them.  Returns a list of [x0, y0, x1, y1] floats."""
    b = np.asarray(bboxs, dtype=np.int64).reshape(-1, 4)
    if b.shape[0] == 0:
        return []
    take = rng.random(b.shape[0]) >= outside
    cx, cy = (b[:, 0] + b[:, 2]) // 2 // cell[0], (b[:, 1] + b[:, 3]) // 2 // cell[1]
    cells = {}
    for i in np.nonzero(take)[0].tolist():
        cells.setdefault((int(cx[i]), int(cy[i])), []).append(i)
    blocks = []
    for ids in cells.values():
        w = b[ids]
        blocks.append([float(w[:, 0].min()) * scale, float(w[:, 1].min()) * scale, float(w[:, 2].max()) * scale, float(w[:, 3].max()) * scale])
    return [blocks[i] for i in rng.permutation(len(blocks)).tolist()]
