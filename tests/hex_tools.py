"""Helpers for the Q_p hexahedral (C5) tests: map the product's subdomain-major element numbering onto the
oracle's lexicographic numbering of the same structured grid; and the graded (rectilinear) test mesh with its map."""
import numpy as np


def lex_to_product(grid, n, lower, upper):
    """elem_index for the oracle: oracle element (lexicographic i + n0 (j + n1 k)) -> product global id."""
    coords, ev, _ = grid.connectivity()
    v0 = coords[ev[:, 0]]                                   # vertex 0 = lower corner of every hexahedron
    h = (np.asarray(upper, float) - np.asarray(lower, float)) / np.asarray(n, float)
    ijk = np.rint((v0 - np.asarray(lower, float)) / h).astype(np.int64)
    lex = ijk[:, 0] + n[0] * (ijk[:, 1] + n[1] * ijk[:, 2])
    elem_index = np.empty(grid.ne, np.int64)
    elem_index[lex] = np.arange(grid.ne)
    return elem_index


# The graded (rectilinear) test mesh: 5 x 4 x 3 hexahedra on [-1,1] x [0,1.5] x [0.5,2]; x widths in geometric
# ratio 1.7, y widths 1:3:1:2, z widths 2:1:3.  Every axis has its own grading and neighbour ratios reach 3.
def _breakpoints(lower, upper, widths):
    w = np.asarray(widths, float)
    x = lower + (upper - lower) * np.concatenate([[0.0], np.cumsum(w)]) / w.sum()
    x[-1] = upper
    return x


GRADED_NODES = (_breakpoints(-1.0, 1.0, 1.7 ** np.arange(5)), _breakpoints(0.0, 1.5, [1, 3, 1, 2]),
                _breakpoints(0.5, 2.0, [2, 1, 3]))


def graded_hex_mesh(nodes):
    """(coords [nv][3], ev [ne][8]) of the rectilinear grid with per-axis breakpoints nodes[a]: elements
    lexicographic (x fastest), vertices of an element in Dune cube order (bit a of k = upper side of axis a)."""
    nodes = [np.asarray(x, float) for x in nodes]
    m = [x.shape[0] for x in nodes]                          # vertices per axis
    Z, Y, X = np.meshgrid(nodes[2], nodes[1], nodes[0], indexing="ij")
    coords = np.stack([X.ravel(), Y.ravel(), Z.ravel()], 1).copy()
    k, j, i = np.meshgrid(np.arange(m[2] - 1), np.arange(m[1] - 1), np.arange(m[0] - 1), indexing="ij")
    v0 = (i + m[0] * (j + m[1] * k)).ravel()
    ev = np.stack([v0 + (c & 1) + m[0] * ((c >> 1 & 1) + m[1] * (c >> 2)) for c in range(8)], 1).astype(np.int32)
    return coords, ev


def lex_to_product_graded(grid, nodes):
    """elem_index for the oracle on a graded grid: every element's vertex 0 located in the breakpoint arrays."""
    coords, ev, _ = grid.connectivity()
    v0 = coords[ev[:, 0]]
    n = [len(x) - 1 for x in nodes]
    ijk = []
    for a in range(len(nodes)):
        x = np.asarray(nodes[a], float)
        mid = 0.5 * (x[:-1] + x[1:])                         # vertex 0 = breakpoint i lies in (mid[i-1], mid[i])
        ijk.append(np.searchsorted(mid, v0[:, a]))
        assert np.array_equal(x[ijk[a]], v0[:, a])           # and it is that breakpoint, exactly
    lex = ijk[0] + n[0] * ijk[1] + (n[0] * n[1] * ijk[2] if len(nodes) == 3 else 0)
    elem_index = np.empty(grid.ne, np.int64)
    elem_index[lex] = np.arange(grid.ne)
    return elem_index
