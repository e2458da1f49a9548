"""CPU: the numpy doubling that the GPU jump-table tests compare against (astar_jump_oracle.jump_tables) agrees with the plain
walk of the next-hop map (astar_oracle.walk), so the yardstick is checked without a device."""
import numpy as np
import pytest

import astar_jump_oracle as J
import astar_maps as M
import astar_oracle as O


def _maps():
    return {"spiral24": M.spiral(24), "walled_off": J.walled_off()}


@pytest.mark.parametrize("name", ["spiral24", "walled_off"])
def test_doubling_agrees_with_the_walk(name):
    h, r, thr, res, goal = _maps()[name]
    H, W = h.shape
    _, nxt = O.solve(h, r, thr, res, goal)
    hops, jump = J.jump_tables(nxt)
    assert jump.shape == (J.num_levels(H * W), H * W)
    reach = 0
    for c in range(H * W):
        path = O.walk(nxt, (c % W, c // W))
        if path is None:
            assert hops[c // W, c % W] == -1, c
            assert O.walk(nxt, (int(jump[-1][c]) % W, int(jump[-1][c]) // W)) is None       # still among the cells without a path
            continue
        reach += 1
        assert hops[c // W, c % W] == len(path) - 1, c
        nodes = [iy * W + ix for ix, iy in path]
        for k, lvl in enumerate(jump):                 # 2^k hops on, or the goal once the path has ended
            assert lvl[c] == nodes[min(1 << k, len(nodes) - 1)], (c, k)
        for i in {0, min(1, len(nodes) - 1), len(nodes) // 2, len(nodes) - 1}:   # any node by decomposing its index over the levels
            assert J.node(jump, c, i) == nodes[i], (c, i)
    if name == "walled_off":
        assert 0 < reach < H * W and hops[17, 14] == -1 and hops[5, 5] > 0
    else:
        assert hops.max() == 286 and reach == H * W


def test_num_levels_addresses_every_node_index():
    for cells, want in ((1, 1), (2, 1), (3, 2), (97, 7), (1089, 11), (4096, 12), (4097, 13), (1 << 18, 18)):
        assert J.num_levels(cells) == want
        assert (1 << J.num_levels(cells)) >= cells
