"""Preconditions of the projection grid tests (tests/project_grid_cases.py), on the host.

test_gpu_project_grid.py cannot observe how many tiles a workgroup of project_tile_kernel walked or whether a wave of
project_csr_kernel took a second chunk; it relies on the launch arithmetic restated in project_grid_cases.py.  These
tests assert that the restated constants are the sources', that the closed forms agree with the loops walked one by one,
and that on 256 CUs -- and on other CU counts at which apply_grid's G is still above the 512-part cap -- the meshes have
the facts the GPU tests need.  CPU only."""
import os
import re

import numpy as np
import pytest

import hdd_amd as H
import project_grid_cases as PG
from cases import SPE10_LOWER, SPE10_UPPER

KERNELS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dune-hdd_amd", "csrc", "kernels")


def _source(name):
    with open(os.path.join(KERNELS, name)) as f:
        return f.read()


def test_restated_constants_come_from_the_sources():
    pk, ap, ab = _source("project_kernels.hh"), _source("apply_plan.hh"), _source("abi_project.hip")
    assert re.search(r"constexpr int PROJECT_BLOCKS = %d;" % PG.PROJECT_BLOCKS, pk)
    assert "constexpr int project_csr_rows(int G) { return G == 8 ? %d : %d; }" % (PG.CSR_ROWS["csr8"], PG.CSR_ROWS["csr64"]) in pk
    assert "ch += int64_t(gridDim.x) * 4" in pk and "base += int64_t(gridDim.x) * 256" in pk
    assert "dot_grid(ctx, P, dev::PROJECT_BLOCKS)" in ab and "4 * dev::project_csr_rows(P.short_rows ? 8 : 64)" in ab
    assert "std::min<int64_t>((n + 255) / 256, dev::PROJECT_BLOCKS)" in ab
    assert "std::min<int64_t>(8, (160 * 1024) / P.image_bytes())" in ap and "return G > max_parts ? max_parts & ~int64_t(7) : G;" in ap
    assert H.MAX_COMP == PG.MAX_COMP
    # ApplyImage<NB, NF>::BYTES (apply_kernels.hh) -> LDS images per CU
    for kind, nb in (("p1", 3), ("q1", 4)):
        bb = nb * nb
        image_bytes = ((32 * bb * (nb + 1) + bb % 2 + 63) // 64) * 64 * 16
        assert image_bytes == {"p1": 19456, "q1": 40960}[kind]
        assert max(1, min(8, 160 * 1024 // image_bytes)) == PG.PER_CU[kind]


@pytest.mark.parametrize("G,n_tiles", [(8, 9), (8, 64), (16, 17), (512, 513), (512, 515), (512, 518), (512, 1036), (512, 4099), (24, 7)])
def test_tile_range_closed_form(G, n_tiles):
    """tiles_per_wave against tile_range walked workgroup by workgroup: every tile once"""
    walk = PG.tile_walk(min(G, n_tiles), n_tiles)
    assert sorted(t for w in walk for t in w) == list(range(n_tiles))
    assert [len(w) for w in walk] == PG.tiles_per_wave(min(G, n_tiles), n_tiles).tolist()


def test_project_parts_formula():
    assert PG.project_parts(256, "p1", 7) == 7 and PG.project_parts(256, "p1", 512) == 512
    assert PG.project_parts(256, "p1", 513) == 512 and PG.project_parts(256, "q1", 1000) == 512
    assert PG.project_parts(32, "p1", 1036) == 256 and PG.project_parts(32, "q1", 1036) == 128
    assert PG.project_parts(256, "csr8", 1) == 1 and PG.project_parts(256, "csr8", 129) == 2
    assert PG.project_parts(256, "csr8", 65536) == 512 and PG.project_parts(256, "csr8", 65537) == 512
    assert PG.project_parts(256, "csr64", 32768) == 512 and PG.project_parts(256, "csr64", 64) == 1
    # a second chunk exactly above 512 x 4 x 32 (16) rows
    assert PG.chunks_per_wave(512, 65536, 32).max() == 1 and PG.chunks_per_wave(512, 65537, 32).max() == 2
    assert PG.chunks_per_wave(512, 32768, 16).max() == 1 and PG.chunks_per_wave(512, 32769, 16).max() == 2
    assert PG.inner_passes_per_wave(PG.INNER_SWEEP).max() == 1 and PG.inner_passes_per_wave(PG.INNER_SWEEP + 1).max() == 2


CU_COUNTS = [PG.MI355X_CUS, 304, 192]


@pytest.mark.parametrize("n_cu", CU_COUNTS)
def test_p1_mesh_facts(n_cu):
    f = PG.p1_size(n_cu)
    assert PG.p1_conditions(f) and (f["nx"], f["ny"]) == (130, 255)
    assert PG.apply_tile_grid(n_cu, "p1") > PG.PROJECT_BLOCKS
    t, s = f["tile"], f["sub_tile"]
    assert (t["n_el"], t["n_tiles"], t["n_tiles"] % 8, t["last_tile"], t["parts"]) == (66300, 1036, 4, 60, 512)
    assert t["waves_at"] == {2: 500, 3: 12} and t["last_tile_position"] == 2
    assert f["csr"]["rows"] == 198900 and f["csr"]["min_chunks"] == 3 and f["csr"]["max_chunks"] == 4
    assert f["sub_start"] == 33150 and f["sub_start"] % 64 == 62
    assert (s["n_el"], s["n_tiles"], s["n_tiles"] % 8, s["parts"]) == (33150, 518, 6, 512)
    assert s["waves_at"] == {1: 506, 2: 6} and s["last_tile_position"] == 1
    assert f["sub_csr"]["rows"] == 99450 and f["sub_csr"]["chunks"] == 3108 and f["sub_csr"]["waves"] == 2048


@pytest.mark.parametrize("n_cu", CU_COUNTS)
def test_q1_mesh_facts(n_cu):
    f = PG.q1_size(n_cu)
    assert PG.q1_conditions(f) and (f["nx"], f["ny"]) == (182, 181)
    assert PG.apply_tile_grid(n_cu, "q1") > PG.PROJECT_BLOCKS
    t = f["tile"]
    assert (t["n_el"], t["n_tiles"], t["n_tiles"] % 8, t["last_tile"], t["parts"]) == (32942, 515, 3, 46, 512)
    assert t["waves_at"] == {1: 509, 2: 3} and t["last_tile_position"] == 1
    assert f["csr"]["rows"] == 131768 and f["csr"]["chunks"] == 4118 > 2 * f["csr"]["waves"] == 4096


def test_hex_mesh_facts():
    f = PG.hex_size()
    assert PG.hex_conditions(f) and f["n"] == (16, 16, 17)
    assert f["rows"] == 34816 and f["csr"]["chunks"] == 2176 and f["csr"]["waves"] == 2048
    assert int((PG.chunks_per_wave(512, f["rows"], 16) == 2).sum()) == 128
    # the restated entry count is the grid's: 8 (1 + interior faces) entries in each of an element's 8 rows
    loc = H.Grid.structured3d(f["n"], degree=1).local()
    assert loc.n_own == f["rows"] // 8 and 64 * int((1 + (loc.neighbors >= 0).sum(axis=0)).sum()) == f["nnz"]
    assert f["nnz"] // f["rows"] > 32


def test_a_device_below_the_cap_fails_loudly():
    """fewer CUs than 512 parts need: no mesh is returned, rather than one that stays inside one pass"""
    with pytest.raises(AssertionError, match="no P1 projection mesh"):
        PG.p1_size(32)
    with pytest.raises(AssertionError, match="no Q1 projection mesh"):
        PG.q1_size(64)
    assert not PG.tile_conditions(PG.tile_facts(256, "p1", 400), 1, 1)         # the largest tile case of test_gpu_project.py
    assert not PG.inner_conditions(4097) and all(PG.inner_conditions(n) for n in PG.INNER_N)
    assert not PG.inner_conditions(PG.INNER_SWEEP)


def test_the_grids_number_their_subdomains_as_restated():
    f = PG.p1_size(PG.MI355X_CUS)
    g = H.Grid.structured(H.SIMPLEX, f["nx"], f["ny"], SPE10_LOWER, SPE10_UPPER, px=2, py=1)
    assert g.n_sub == 2 and g.ne == f["tile"]["n_el"]
    assert g.subdomain_range(0, 1) == (0, f["sub_start"]) and g.subdomain_range(1, 2) == (f["sub_start"], g.ne)
    loc = g.local()
    assert loc.own_begin == 0 and loc.n_local == g.ne
    assert PG.elem_ptr(loc.neighbors, 3)[f["sub_start"]] % 2 == 1           # an odd base - base_al at subdomain 1's first tile
    assert PG.coupled_pairs(loc.neighbors, [0, f["sub_start"]]) == [(0, 0), (0, 1), (1, 0), (1, 1)]


def test_small_block_cases_start_off_the_tile_boundary():
    """Kuhn 18 x 5 in three slabs of 60 (odd elem_ptr at both inner starts; subdomain 1 has a lower- and a
    higher-numbered neighbour) and the cube 16 x 12 in 2 x 2 of 48"""
    nx, ny, px = PG.P1_SMALL_BLOCK
    g = H.Grid.structured(H.SIMPLEX, nx, ny, SPE10_LOWER, SPE10_UPPER, px=px, py=1)
    starts = [g.subdomain_range(s, s + 1)[0] for s in range(g.n_sub)]
    assert starts == [0, 60, 120]
    loc = g.local()
    ep = PG.elem_ptr(loc.neighbors, 3)
    assert all(ep[a] % 2 == 1 and a % 64 != 0 for a in starts[1:])
    assert PG.coupled_pairs(loc.neighbors, starts) == [(0, 0), (0, 1), (1, 0), (1, 1), (1, 2), (2, 1), (2, 2)]
    g = H.Grid.structured(H.CUBE, 16, 12, SPE10_LOWER, SPE10_UPPER, px=2, py=2)
    starts = [g.subdomain_range(s, s + 1)[0] for s in range(g.n_sub)]
    assert starts == [0, 48, 96, 144]
    pairs = PG.coupled_pairs(g.local().neighbors, starts)
    assert len(pairs) == 12 and (1, 2) not in pairs and (3, 0) not in pairs       # the diagonal neighbours do not couple
