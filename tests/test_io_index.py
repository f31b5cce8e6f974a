"""The index arithmetic of the separate unpack / Phred stages (csrc/io_kernels.hip), replayed in numpy over every row
width the launchers admit and every element of a tile.  Inside a tile the kernels split an element index e into site,
member and genotype with two multiply-high divisions instead of integer divisions; the split is only right while
tile * 3 * members stays below 2^16.  Up to 170 members a tile holds 128 sites; wider rows take fewer sites per tile
(before that the launchers refused them, and `r / 3` was `(r * 171) >> 9`, which is wrong from r = 513 on)."""
import os
import re

import numpy as np

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "famseq_amd", "csrc", "io_kernels.hip")


def constants():
    src = open(SRC).read()
    tile = int(re.search(r"constexpr int kTileSites = (\d+);", src).group(1))
    most = int(re.search(r"constexpr int kMaxIoMembers = (\d+);", src).group(1))
    # the kernels' own spellings, so that a change of formula shows up here (a mere reformatting of these lines fails too:
    # then update the strings, after checking that the arithmetic replayed below is still what the kernels do)
    assert "i = div_small(r, m3), g = r - 3 * i;" in src and "k = div_small(r, m3), g = r - 3 * k;" in src
    assert src.count("tile = tile_sites(w3)") == 2 and "0xFFFFu / w3 < kTileSites ? 0xFFFFu / w3 : kTileSites" in src
    return tile, most


def magic_for(d):
    return (0xFFFFFFFF // d + 1) & 0xFFFFFFFF  # (unsigned arithmetic: d = 1 wraps to 0, and no row has w3 = 1)


def tile_sites(w3, k_tile):
    return min(0xFFFF // w3, k_tile)


def test_tile_shape_at_the_edges():
    k_tile, most = constants()
    assert tile_sites(3 * 170, k_tile) == 128  # unchanged up to 170 members: same tiles, same launches as before
    assert tile_sites(3 * 171, k_tile) == 127 and tile_sites(3 * 200, k_tile) == 109
    assert tile_sites(3 * most, k_tile) == 1 and 3 * most <= 0xFFFF < 3 * (most + 1)


def test_site_member_genotype_split_is_exact_over_the_launchers_domain():
    k_tile, most = constants()
    e_all = np.arange(1 << 16, dtype=np.int64)
    m3 = magic_for(3)
    r_all = (e_all * m3) >> 32
    # r / 3 for every r a row can hold (r < 3 * most <= 65535)
    assert np.array_equal(r_all[: 3 * most], e_all[: 3 * most] // 3)
    for m in range(1, most + 1):
        w3 = 3 * m
        tile = tile_sites(w3, k_tile)
        n = tile * w3  # elements of a whole tile (a ragged last tile is a prefix of it)
        assert 1 <= tile and n < (1 << 16), m
        e = e_all[:n]
        s = (e * magic_for(w3)) >> 32
        r = e - s * w3
        assert r.min() >= 0 and r.max() < w3, m  # s = e / w3 exactly
        i = r_all[r]  # member: the same multiply-high by the magic of 3
        g = r - 3 * i
        assert s[-1] == tile - 1 and g.min() >= 0 and g.max() <= 2 and i.max() == m - 1, m
