"""Sizes of the projection grid tests (test_project_grid_cases.py on the host, test_gpu_project_grid.py on the device):
the launch arithmetic of hdd_operator_project / hdd_vectors_inner restated in numpy, and the meshes at which the loops
of project_tile_kernel, project_csr_kernel and inner_kernel take more than one round.

Restated from the sources:
  apply_grid / dot_grid (apply_plan.hh), project_parts (abi_project.hip):
      tile kernel: G = max(8, (n_cu per_cu) & ~7) workgroups, per_cu = 8 (P1 image) or 4 (Q1 image), at most the tile
      count, and at most PROJECT_BLOCKS = 512 parts; CSR kernel: ceil(rows / (4 RW)) workgroups of four waves, RW = 32
      rows per wave pass (<8>) or 16 (<64>), at least 1 and at most 512 -- no CU count in it.
  tile_range (swipdg_persistent.hh): with fewer workgroups than tiles, workgroup b walks the eighth b & 7 of the tile
      range from position b >> 3 in steps of G / 8.
  project_csr_kernel: wave w of 4 parts walks the chunks w, w + 4 parts, ... of RW rows.
  hdd_vectors_inner: min(ceil(n / 256), 512) workgroups, a wave pass is 64 entries, a sweep is 256 parts entries.

Every mesh choice is a function of the CU count and returns the facts it satisfies; a device on which the issue's mesh
misses a fact gets the next mesh that has it, or an AssertionError -- never a mesh that stays inside one pass.

Only numpy here; nothing needs a GPU or the library."""
import numpy as np

PROJECT_BLOCKS = 512        # project_kernels.hh
MAX_COMP = 8                # hdd.h: HDD_MAX_COMP
MI355X_CUS = 256
PER_CU = {"p1": 8, "q1": 4}                 # LDS images of apply_grid per CU: 160 KB / 19,456 B (capped at 8), / 40,960 B
CSR_ROWS = {"csr8": 32, "csr64": 16}        # project_csr_rows: rows of a wave pass
INNER_SWEEP = PROJECT_BLOCKS * 256          # entries of one sweep of inner_kernel at its cap


def apply_tile_grid(n_cu, kind):
    """G of apply_grid before the tile count caps it"""
    return max(8, (n_cu * PER_CU[kind]) & ~7)


def project_parts(n_cu, kind, n):
    """gridDim.x of hdd_operator_project: kind "p1" / "q1" with n tiles, "csr8" / "csr64" with n rows (n > 0)"""
    assert n > 0
    if kind in PER_CU:
        G = min(apply_tile_grid(n_cu, kind), n)
        return PROJECT_BLOCKS & ~7 if G > PROJECT_BLOCKS else G
    per_wg = 4 * CSR_ROWS[kind]
    return max(1, min(-(-n // per_wg), PROJECT_BLOCKS))


def tile_walk(G, n_tiles):
    """tile_range: the tiles of each of the G workgroups, in the order it walks them"""
    if G >= n_tiles:
        return [[b] for b in range(G)]
    assert G % 8 == 0
    out = []
    for b in range(G):
        x, w, gx = b & 7, b >> 3, G >> 3
        out.append(list(range(n_tiles * x // 8 + w, n_tiles * (x + 1) // 8, gx)))
    return out


def tiles_per_wave(G, n_tiles):
    """how many tiles each workgroup (= wave) of the tile kernel walks (closed form of tile_walk)"""
    if G >= n_tiles:
        return np.ones(n_tiles, np.int64)
    b = np.arange(G)
    x, w, gx = b & 7, b >> 3, G >> 3
    s0, s1 = n_tiles * x // 8, n_tiles * (x + 1) // 8
    return np.maximum(0, -(-(s1 - s0 - w) // gx))


def chunks_per_wave(parts, rows, rw):
    """project_csr_kernel: chunks of rw rows that each of the 4 parts waves takes"""
    waves = 4 * parts
    chunks = -(-rows // rw)
    return np.maximum(0, -(-(chunks - np.arange(waves)) // waves))


def inner_parts(n):
    return min(-(-n // 256), PROJECT_BLOCKS)


def inner_passes_per_wave(n):
    """inner_kernel: 64-entry passes of each of the 4 parts waves"""
    waves = 4 * inner_parts(n)
    return np.maximum(0, -(-(-(-n // 64) - np.arange(waves)) // waves))


def tile_facts(n_cu, kind, n_el):
    """what the tile kernel does on a range of n_el elements"""
    n_tiles = -(-n_el // 64)
    parts = project_parts(n_cu, kind, n_tiles)
    walk = tile_walk(parts, n_tiles)
    per_wave = tiles_per_wave(parts, n_tiles)
    assert [len(w) for w in walk] == per_wave.tolist() and sorted(t for w in walk for t in w) == list(range(n_tiles))
    (last_pos,) = [w.index(n_tiles - 1) for w in walk if n_tiles - 1 in w]
    return dict(n_el=n_el, n_tiles=n_tiles, parts=parts, G=apply_tile_grid(n_cu, kind), last_tile=n_el - 64 * (n_tiles - 1),
                min_tiles=int(per_wave.min()), max_tiles=int(per_wave.max()),
                waves_at={int(k): int((per_wave == k).sum()) for k in np.unique(per_wave)},
                last_tile_position=last_pos, eighths=[n_tiles * (x + 1) // 8 - n_tiles * x // 8 for x in range(8)])


def csr_facts(kind, rows):
    parts = project_parts(0, kind, rows)
    per_wave = chunks_per_wave(parts, rows, CSR_ROWS[kind])
    assert per_wave.sum() == -(-rows // CSR_ROWS[kind])
    return dict(rows=rows, parts=parts, waves=4 * parts, chunks=int(per_wave.sum()), min_chunks=int(per_wave.min()),
                max_chunks=int(per_wave.max()), last_chunk=rows - CSR_ROWS[kind] * (int(per_wave.sum()) - 1))


def tile_conditions(f, min_tiles, max_tiles):
    """a range whose workgroups walk min_tiles .. max_tiles tiles each at the 512-part cap: the cap is reached and lies
    below the tile count, the XCD eighths are uneven, the last tile is partial and is not its wave's first"""
    return (f["parts"] == PROJECT_BLOCKS and f["n_tiles"] > f["parts"]
            and f["min_tiles"] == min_tiles and f["max_tiles"] == max_tiles and f["n_tiles"] % 8 != 0
            and len(set(f["eighths"])) > 1 and 0 < f["last_tile"] < 64 and f["last_tile_position"] > 0)


def p1_facts(n_cu, nx, ny):
    """Kuhn nx x ny whole and in px = 2 x-slabs of nx / 2 columns (subdomain s holds elements [s n_el / 2, ..))"""
    n_el = 2 * nx * ny
    return dict(nx=nx, ny=ny, tile=tile_facts(n_cu, "p1", n_el), csr=csr_facts("csr8", 3 * n_el),
                sub_start=n_el // 2, sub_tile=tile_facts(n_cu, "p1", n_el // 2), sub_csr=csr_facts("csr8", 3 * (n_el // 2)))


def p1_conditions(f):
    """whole mesh: two and three tiles per wave; a subdomain: starts inside a tile of the global numbering, one and two
    tiles per wave; CSR: a second chunk for every wave of the whole mesh and for some of a subdomain's"""
    return (f["nx"] % 2 == 0 and tile_conditions(f["tile"], 2, 3) and f["sub_start"] % 64 != 0 and tile_conditions(f["sub_tile"], 1, 2) and f["csr"]["parts"] == PROJECT_BLOCKS and f["csr"]["min_chunks"] >= 2
            and f["sub_csr"]["parts"] == PROJECT_BLOCKS and f["sub_csr"]["max_chunks"] >= 2)


def p1_size(n_cu):
    """Kuhn 130 x 255, or the next ny with p1_conditions on this CU count"""
    for ny in range(255, 1024):
        f = p1_facts(n_cu, 130, ny)
        if p1_conditions(f):
            return f
    raise AssertionError("no P1 projection mesh for %d CUs" % n_cu)


def q1_facts(n_cu, nx, ny):
    return dict(nx=nx, ny=ny, tile=tile_facts(n_cu, "q1", nx * ny), csr=csr_facts("csr8", 4 * nx * ny))


def q1_conditions(f):
    """one and two tiles per wave; more than two CSR chunks per wave"""
    return tile_conditions(f["tile"], 1, 2) and f["csr"]["parts"] == PROJECT_BLOCKS and f["csr"]["min_chunks"] >= 2 \
        and f["csr"]["chunks"] > 2 * f["csr"]["waves"]


def q1_size(n_cu):
    """cube 182 x 181, or the next ny with q1_conditions on this CU count"""
    for ny in range(181, 1024):
        f = q1_facts(n_cu, 182, ny)
        if q1_conditions(f):
            return f
    raise AssertionError("no Q1 projection mesh for %d CUs" % n_cu)


def hex_facts(n):
    """Q1 hexahedra n[0] x n[1] x n[2]: 8 rows per element, 8 (1 + interior faces) entries per row"""
    n_el = n[0] * n[1] * n[2]
    faces = sum(2 * (m - 1) * n_el // m for m in n)        # interior faces, counted from both sides
    return dict(n=tuple(n), rows=8 * n_el, nnz=64 * (n_el + faces), csr=csr_facts("csr64", 8 * n_el))


def hex_conditions(f):
    """project_csr_kernel<64> is the kernel taken (plan_apply: nnz / rows > 32) and some of its waves take two chunks"""
    return f["nnz"] // f["rows"] > 32 and f["csr"]["parts"] == PROJECT_BLOCKS and f["csr"]["max_chunks"] >= 2 \
        and f["csr"]["chunks"] > f["csr"]["waves"]


def hex_size(n_cu=MI355X_CUS):
    """16 x 16 x 17, or the next depth with hex_conditions (the CSR grid does not depend on the CU count)"""
    for nz in range(17, 64):
        f = hex_facts((16, 16, nz))
        if hex_conditions(f):
            return f
    raise AssertionError("no hexahedral projection mesh")


P1_SMALL_BLOCK = (18, 5, 3)     # Kuhn 18 x 5 in px = 3 slabs of 60 elements: starts 60 and 120, both with an odd elem_ptr


def elem_ptr(neighbors, nb):
    """hdd_dg_pattern_fill's elem_ptr of a whole-grid view: nb^2 (1 + interior faces) values per element;
    neighbors: [nf][n], boundary faces negative"""
    return np.concatenate([[0], np.cumsum(nb * nb * (1 + (neighbors >= 0).sum(axis=0)))])


def coupled_pairs(neighbors, starts):
    """the (ss, nn) whose operator has a block: subdomains ss = the slab [starts[ss], starts[ss + 1]) of the elements"""
    starts = np.asarray(starts)
    own = np.searchsorted(starts, np.arange(neighbors.shape[1]), side="right") - 1
    pairs = {(int(s), int(s)) for s in np.unique(own)}
    for f in range(neighbors.shape[0]):
        m = neighbors[f] >= 0
        pairs |= set(zip(own[m].tolist(), own[neighbors[f][m]].tolist()))
    return sorted(pairs)


INNER_N = (INNER_SWEEP + 1, 3 * INNER_SWEEP + 77)


def inner_conditions(n):
    """inner_kernel at its 512 parts with a second pass for at least one wave"""
    p = inner_passes_per_wave(n)
    return inner_parts(n) == PROJECT_BLOCKS and n > INNER_SWEEP and p.max() >= 2 and p.sum() == -(-n // 64)
