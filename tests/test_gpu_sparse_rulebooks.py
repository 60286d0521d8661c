"""The HIP rulebook builders (rpc_subm_rulebook, rpc_spconv_rulebook_count + _build) through the C ABI against
brute-force rulebooks (tests/_sparse_cases.py), exactly: every neighbour, the documented output order, the
inverse map, the grid left all -1, on voxel sets that sit on the faces and corners of the volume and on both
sides of the seam between two frames of the linear grid."""
import numpy as np
import pytest
import torch

from robustpointclouds_amd import _ffi
from tests import _sparse_cases as sc
from tests._sparse_hip import MARK, hip_strided, hip_subm, index_grid as _grid

pytestmark = pytest.mark.gpu

RPC_OK, RPC_ERR_WORKSPACE, RPC_ERR_UNSUPPORTED = 0, 2, 3
NS = [1, 2, 130]


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("shape", sc.GRIDS)
def test_subm_rulebook_matches_brute_force(shape, n):
    dev = torch.device("cuda")
    coors = sc.coors_for(shape, n, seed=1)
    grid = _grid(shape, dev)
    nbr = hip_subm(coors, shape, grid).cpu().numpy()
    assert np.array_equal(nbr, sc.subm_rulebook(coors))
    assert np.array_equal(nbr[:, 13], np.arange(n))
    assert bool((grid == -1).all())


def _check_strided(coors, shape, geom, grid):
    n_out, coors_out, nbr_out, nbr_in = hip_strided(coors, shape, geom, grid)
    want_c, want_out, want_in = sc.strided_rulebook(coors, shape, *geom)
    assert n_out == len(want_c)
    coors_out, nbr_out, nbr_in = coors_out.cpu().numpy(), nbr_out.cpu().numpy(), nbr_in.cpu().numpy()
    assert np.array_equal(coors_out, want_c)          # order included: first candidate, ascending r * K + k
    assert np.array_equal(nbr_out, want_out)
    assert np.array_equal(nbr_in, want_in)
    # the two maps are each other's inverse; nothing else is set; every output row is reached
    o, k = np.nonzero(nbr_out >= 0)
    assert (nbr_in[nbr_out[o, k], k] == o).all()
    i, k = np.nonzero(nbr_in >= 0)
    assert (nbr_out[nbr_in[i, k], k] == i).all()
    assert ((nbr_out == -1) | (nbr_out >= 0)).all() and ((nbr_in == -1) | (nbr_in >= 0)).all()
    assert (nbr_out < len(coors)).all() and (nbr_in < n_out).all()
    assert (nbr_out >= 0).any(1).all()
    assert bool((grid == -1).all())


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("geom", sc.GEOMS)
@pytest.mark.parametrize("shape", sc.GRIDS)
def test_strided_rulebook_matches_brute_force(shape, geom, n):
    dev = torch.device("cuda")
    grid = _grid(sc.out_shape(shape, *geom), dev)
    _check_strided(sc.coors_for(shape, n, seed=1), shape, geom, grid)
    # the grid is reusable: another voxel set through the same grid tensor gives its own exact result
    _check_strided(sc.corner_case_coors(shape, 61, seed=5), shape, geom, grid)


@pytest.mark.parametrize("shape", sc.GRIDS)
def test_subm_grid_is_reusable(shape):
    dev = torch.device("cuda")
    grid = _grid(shape, dev)
    for n, seed in ((130, 1), (61, 5)):
        coors = sc.corner_case_coors(shape, n, seed)
        assert np.array_equal(hip_subm(coors, shape, grid).cpu().numpy(), sc.subm_rulebook(coors))
        assert bool((grid == -1).all())


def test_rulebook_argument_handling():
    """Refusals come back as error codes before anything is launched; every buffer is a real device buffer."""
    lib = _ffi.load()
    dev = torch.device("cuda")
    shape = sc.GRIDS[0]
    coors = sc.corner_case_coors(shape, 130, seed=1)
    cd = torch.from_numpy(coors).to(dev)
    n = len(coors)
    grid = _grid(shape, dev)
    st = _ffi.stream_of(cd)
    shp, k5, k3, s2, p1 = (_ffi.int_arr(v) for v in (shape, (5, 5, 5), (3, 3, 3), (2, 2, 2), (1, 1, 1)))
    big = torch.full((n, 125), MARK, dtype=torch.int32, device=dev)
    # ksize (5, 5, 5): 125 offsets, more than the builders hold
    assert lib.rpc_subm_rulebook(_ffi.ptr(cd), n, shp, k5, _ffi.ptr(grid), _ffi.ptr(big), st) == RPC_ERR_UNSUPPORTED
    wsb = lib.rpc_spconv_rulebook_workspace_size(n, 125)
    ws = _ffi.workspace(wsb, dev)
    n_dev = torch.full((1,), MARK, dtype=torch.int32, device=dev)
    oshp = _ffi.int_arr(sc.out_shape(shape, (3, 3, 3), (2, 2, 2), (1, 1, 1)))
    assert lib.rpc_spconv_rulebook_count(_ffi.ptr(cd), n, oshp, k5, s2, p1, _ffi.ptr(grid), _ffi.ptr(n_dev),
                                         _ffi.ptr(ws), wsb, st) == RPC_ERR_UNSUPPORTED
    big_c = torch.full((n, 4), MARK, dtype=torch.int32, device=dev)
    big_in = torch.full((n, 125), MARK, dtype=torch.int32, device=dev)
    assert lib.rpc_spconv_rulebook_build(_ffi.ptr(cd), n, oshp, k5, s2, p1, _ffi.ptr(grid), n, _ffi.ptr(big_c),
                                         _ffi.ptr(big), _ffi.ptr(big_in), _ffi.ptr(ws), st) == RPC_ERR_UNSUPPORTED
    # a workspace one byte short
    need = lib.rpc_spconv_rulebook_workspace_size(n, 27)
    assert 0 < need <= wsb
    assert lib.rpc_spconv_rulebook_count(_ffi.ptr(cd), n, oshp, k3, s2, p1, _ffi.ptr(grid), _ffi.ptr(n_dev),
                                         _ffi.ptr(ws), need - 1, st) == RPC_ERR_WORKSPACE
    # N = 0: nothing to do, nothing written
    assert lib.rpc_subm_rulebook(_ffi.ptr(cd), 0, shp, k3, _ffi.ptr(grid), _ffi.ptr(big), st) == RPC_OK
    torch.cuda.synchronize()
    assert bool((big == MARK).all()) and bool((big_c == MARK).all()) and bool((big_in == MARK).all())
    assert int(n_dev.item()) == MARK and bool((grid == -1).all())
    # and the same buffers still build the exact rulebook afterwards
    assert np.array_equal(hip_subm(coors, shape, grid).cpu().numpy(), sc.subm_rulebook(coors))
