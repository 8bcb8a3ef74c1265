"""The one count-and-place tile body (csrc/nb_scan_dev.h) where its users can go wrong: tile edges, a tie across a tile boundary,
the capacity clamp.  Every expected value is computed in numpy from the definition."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TILE = 1024  # nbscan::TILE


@pytest.mark.parametrize("n", [1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
def test_sparsify_at_the_tile_edges(n):
    """[1, 1, n, 4] volumes of one tile less one voxel, one tile, one tile and a voxel, two tiles and a voxel (and a single voxel):
    every third voxel non-zero, and the first and the last one."""
    from neuralbody_amd import ops

    on = np.zeros(n, dtype=bool)
    on[::3] = True
    on[[0, n - 1]] = True
    vol = np.zeros((1, 1, n, 4), dtype=np.float32)
    vol[0, 0, on, np.arange(n)[on] % 4] = -0.5  # any channel makes a voxel active
    grid, rows_lin, n_rows, cap = ops.sparsify(torch.from_numpy(vol).to(DEV))
    torch.cuda.synchronize()
    lin = np.nonzero(on)[0]
    assert int(n_rows) == lin.size
    assert np.array_equal(rows_lin[:lin.size].cpu().numpy(), lin)
    want = np.full(n, -1, dtype=np.int32)
    want[lin] = np.arange(lin.size)
    assert np.array_equal(grid.cpu().numpy().reshape(-1), want)


@pytest.mark.parametrize("n_verts", [TILE, TILE + 1, TILE + 6])
def test_voxelize_across_a_tile_boundary(n_verts):
    """Vertices 1023 (the last of the first tile) and 1024 (the first of the second) in the same voxel: the later one wins, and the
    rows of the second tile go on where the first tile's end.  One out-of-range coordinate in each tile that has a vertex to spare
    (with 1025 vertices the second tile is vertex 1024 alone, which the tie needs: the 1030-vertex case has both in it)."""
    from neuralbody_amd import ops

    dhw = [16, 16, 16]
    cells = np.random.RandomState(11).permutation(16 ** 3)[:n_verts]  # every vertex a voxel of its own, then the exceptions
    c = np.stack(np.unravel_index(cells, dhw), 1).astype(np.int32)
    c[700] = c[10]  # a tie inside a tile
    if n_verts > TILE:
        c[TILE] = c[TILE - 1]
    c[5] = [16, 0, 0]
    if n_verts > TILE + 3:
        c[TILE + 3] = [0, -1, 3]
    grid, rows_vert, rows_lin, n_rows = ops.enc_voxelize(torch.from_numpy(c).to(DEV), dhw)
    torch.cuda.synchronize()
    winner = {}  # voxel -> the last vertex in it
    for v, (d, h, w) in enumerate(c.tolist()):
        if 0 <= d < 16 and 0 <= h < 16 and 0 <= w < 16:
            winner[(d * 16 + h) * 16 + w] = v
    want_vert = np.array(sorted(winner.values()))
    k = want_vert.size
    assert int(n_rows) == k == len(winner)
    assert 10 not in want_vert and 700 in want_vert and (n_verts == TILE or (TILE - 1 not in want_vert and TILE in want_vert))
    rv, rl = rows_vert[:k].cpu().numpy(), rows_lin[:k].cpu().numpy()
    assert np.all(np.diff(rv) > 0) and np.array_equal(rv, want_vert)
    assert np.array_equal(rl, (c[rv, 0] * 16 + c[rv, 1]) * 16 + c[rv, 2])
    want_grid = np.full(16 ** 3, -1, dtype=np.int32)
    want_grid[rl] = np.arange(k)
    assert np.array_equal(grid.cpu().numpy().reshape(-1), want_grid)


def _clamped(marked, n_cells, cap):
    """The capacity rule: the `cap` lowest marked cells numbered in order, -1 in every other cell."""
    want = np.full(n_cells, -1, dtype=np.int32)
    want[marked[:cap]] = np.arange(cap)
    return want


def test_downsample_index_clamps_to_its_capacity():
    """Three voxels at odd coordinates mark 8 output cells each; a declared capacity of one input row allows 8 rows."""
    from neuralbody_amd import ops

    vox = np.array([[1, 1, 1], [15, 17, 9], [29, 5, 27]])
    in_lin = torch.from_numpy(((vox[:, 0] * 32 + vox[:, 1]) * 32 + vox[:, 2]).astype(np.int32)).to(DEV)
    n_in = torch.tensor([3], dtype=torch.int32, device=DEV)
    og, ol, no, nmax, odhw = ops.enc_downsample_index(in_lin, n_in, 1, [32, 32, 32])
    torch.cuda.synchronize()
    assert nmax == 8 and odhw == [16, 16, 16]
    marked = sorted({(z * 16 + y) * 16 + x for d, h, w in vox.tolist()
                     for z in (d >> 1, (d + 1) >> 1) for y in (h >> 1, (h + 1) >> 1) for x in (w >> 1, (w + 1) >> 1)})
    assert len(marked) == 24
    assert int(no) == 8
    assert ol[:8].cpu().tolist() == marked[:8]
    assert np.array_equal(og.cpu().numpy().reshape(-1), _clamped(np.array(marked), 16 ** 3, 8))


def test_sparsify_clamps_to_its_capacity():
    """nb_sparsify with room for 3 rows on a volume with 7 active voxels: the 3 lowest are numbered, nothing is written behind
    rows_lin[3]."""
    from neuralbody_amd import _lib, ops

    dhw, c = [2, 3, 5], 4
    active = np.array([2, 3, 9, 14, 15, 22, 29])
    vol = np.zeros((30, c), dtype=np.float32)
    vol[active, active % c] = 1.0
    vol_d = torch.from_numpy(vol).to(DEV)
    grid = torch.empty(dhw, dtype=torch.int32, device=DEV)
    rows_lin = torch.full((8,), -7, dtype=torch.int32, device=DEV)
    n_rows = torch.zeros(1, dtype=torch.int32, device=DEV)
    scratch = ops.scan_scratch(30, DEV)
    _lib.check(_lib.lib().nb_sparsify(_lib.ptr(vol_d), (C.c_int32 * 3)(*dhw), c, _lib.ptr(grid), _lib.ptr(rows_lin), _lib.ptr(n_rows),
                                      3, _lib.ptr(scratch), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "nb_sparsify")
    torch.cuda.synchronize()
    assert int(n_rows) == 3
    assert rows_lin.cpu().tolist() == active[:3].tolist() + [-7] * 5
    assert np.array_equal(grid.cpu().numpy().reshape(-1), _clamped(active, 30, 3))


def test_exclusive_scan_beyond_the_two_kernel_form():
    """nb_exclusive_scan on more than 4096 tiles (nb_image_assemble's mask positions over 4.3 Mi pixels): the tile totals get their
    own pass.  A handful of masked pixels at known places, either side of tile and of 256-tile boundaries: pixel p of rank r shows
    rgb_map[r], every other pixel the background."""
    from neuralbody_amd import ops

    n = 4200 * TILE + 3
    lin = torch.tensor([0, TILE - 1, TILE, 256 * TILE - 1, 256 * TILE, 1 << 20, (1 << 22) + 5, n - 1], device=DEV)
    mask = torch.zeros(n, dtype=torch.uint8, device=DEV)
    mask[lin] = 1
    rgb = (torch.arange(3 * lin.numel(), dtype=torch.float32, device=DEV) + 1).reshape(-1, 3)
    img, _ = ops.image_assemble(mask, rgb)
    torch.cuda.synchronize()
    assert torch.equal(img[lin], rgb)
    assert int((img != 0).any(1).sum()) == lin.numel()
