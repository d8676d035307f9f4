"""A numpy model of the per-ray exact episode's bookkeeping (rt2_k5_resident.h
exact_window_lanes): the compaction of a window's hot masks into rounds of 32
triangle indices, the bit <-> MFMA-row map, and the pack / swap that turns the
transposed products' sign bits into one 32-bit mask per ray.  The arithmetic
of the products is not modelled: a product's sign is given as a boolean."""
import numpy as np


def row_of_bit(b):
    """The row of the synthetic group that bit b of a ray's mask comes from."""
    return 8 * ((b & 15) >> 2) + 4 * (b >> 4) + (b & 3)


def bit_of_row(r):
    return 16 * ((r >> 2) & 1) + 4 * (r >> 3) + (r & 3)


def compact(masks, gw, n_tris):
    """The kernel's walk: masks[j] is group gw + j's 32-bit hot mask; the
    scene's last group is cut to n_tris; groups ascending, bits ascending, 32
    per round.  Returns the rounds, each a list of triangle indices."""
    masks = [int(m) for m in masks]
    if n_tris & 31:
        j = (n_tris >> 5) - gw
        if 0 <= j < len(masks):
            masks[j] &= (1 << (n_tris & 31)) - 1
    hotg = sum(1 << j for j, m in enumerate(masks) if m)
    rounds, m, gj = [], 0, 0
    while True:
        lst = []
        while len(lst) < 32:
            if not m:
                if not hotg:
                    break
                gj = (hotg & -hotg).bit_length() - 1
                hotg &= hotg - 1
                m = masks[gj]
            lst.append(32 * (gw + gj) + (m & -m).bit_length() - 1)
            m &= m - 1
        if not lst:
            break
        rounds.append(lst)
        if len(lst) < 32:
            break
    return rounds


def ray_masks(passes, upper=True):
    """One round.  passes[ray, s]: ray (0..63) passes the filter on the round's
    s-th triangle (s < c <= 32).  Follows the data through the kernel: slot s
    sits in row row_of_bit(s); lane l of block R's transposed product holds ray
    32 R + (l & 31), register i = row 8 (i >> 2) + 4 (l >> 5) + (i & 3); register
    i goes to bit i of the block's 16-bit mask; v_permlane32_swap exchanges
    block 0's lanes 32..63 with block 1's lanes 0..31.  Returns the 64 masks."""
    c = passes.shape[1]
    slot_of_row = [bit_of_row(r) for r in range(32)]  # the gather: row r holds slot bit_of_row(r)
    mk = np.zeros((2, 64), dtype=np.uint64)
    for R in range(2 if upper else 1):
        for lane in range(64):
            ray = 32 * R + (lane & 31)
            for i in range(16):
                row = 8 * (i >> 2) + 4 * (lane >> 5) + (i & 3)
                s = slot_of_row[row]
                bit = bool(passes[ray, s]) if s < c else True  # slots past the count: any record
                mk[R, lane] |= np.uint64(int(bit) << i)
    x, y = mk[0].copy(), mk[1].copy()
    x[32:], y[:32] = mk[1][:32], mk[0][32:]
    pm = (x | (y << np.uint64(16))) & np.uint64((1 << c) - 1)
    return pm.astype(np.uint64)
