#!/usr/bin/env python3
"""Search for dp_w4's body-part row layout (dragposer_amd/csrc/dp_w4.h): which items go to side A (block A of layer 2) and which to
side B, so that the two blocks together run the fewest K-groups of layer 2.  An item's K-groups are the aligned groups of 4 hidden
channels in which its rows of the folded A2 = (W2 . M2) U2 are non-zero (the SkeletonConv mask and the 0/1 unpooling make them exact
zeros); a block runs the union of its items' groups.

Only the side of an item matters for the count, so the search is exhaustive over block A's group set GA (2^15 sets): every item whose
groups lie inside GA may go to A, the rest go to B; among the items that may, A takes as many as it has slots (more on A never grows B's
union).  Constraints of the kernel: the root is side A of quad 0 and alone there (stage G sums the root table on that quad), so side A
has 16 slots and side B 15; with --disp-on-b the displacement must be a side-B item (the dense kernel's rule).
Usage: tools/w4_placement.py [model.npz]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NJ, DISP = 22, 22


def item_groups(path):
    z = np.load(path)
    W = z["decoder.layers.2.1.weight"][..., 0] * z["decoder.layers.2.1.mask"][..., 0]
    nz = (np.abs(W) > 0).astype(np.int64) @ (np.abs(z["decoder.layers.2.0.weight"]) > 0).astype(np.int64)  # [92][60]
    par = z["parents"]
    seen, virt = set(), []
    for k in range(1, NJ):
        p = int(par[k])
        if p and p in seen:
            virt.append(p)  # a virtual item per extra child bone: a copy of the joint's rows
        seen.add(p)
    rows = {j: nz[4 * j:4 * j + 4] for j in range(NJ)}
    rows[DISP] = nz[88:92]
    for v, j in enumerate(virt):
        rows[23 + v] = rows[j]
    return {it: sum(1 << k for k in range(15) if r[:, 4 * k:4 * k + 4].any()) for it, r in rows.items()}


def search(groups, disp_on_b):
    items = sorted(groups)
    best = None
    for ga in range(1 << 15):
        if groups[0] & ~ga:
            continue  # the root is a side-A item
        fit = [it for it in items if it != 0 and not (groups[it] & ~ga) and not (disp_on_b and it == DISP)]
        a = [0] + fit[:15]  # (when more fit than there are slots, the ones left over go to B; counted below)
        b = [it for it in items if it not in a]
        if len(b) > 15:
            continue
        gb = 0
        for it in b:
            gb |= groups[it]
        ga_used = 0
        for it in a:
            ga_used |= groups[it]
        cost = bin(ga_used).count("1") + bin(gb).count("1")
        if best is None or cost < best[0]:
            best = (cost, a, b, ga_used, gb)
    return best


def fmt(mask):
    return [k for k in range(15) if mask >> k & 1]


if __name__ == "__main__":
    g = item_groups(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "dragposer_amd", "data", "model_dancedb.npz"))
    for disp_on_b in (True, False):
        cost, a, b, ga, gb = search(g, disp_on_b)
        print(f"displacement {'on side B only' if disp_on_b else 'on either side'}: {cost} K-groups "
              f"({len(fmt(ga))} + {len(fmt(gb))}, {4 * cost} MFMAs of layer 2 against 120)")
        print(f"  side A items {a}: groups {fmt(ga)}")
        print(f"  side B items {b}: groups {fmt(gb)}")
