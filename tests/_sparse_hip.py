"""The HIP rulebook builders called through the C ABI, for the sparse rulebook and kernel tests."""
import torch

from robustpointclouds_amd import _ffi
from tests import _sparse_cases as sc

MARK = -7    # fill of every output buffer: an entry the builder did not write shows


def index_grid(shape, dev):
    return torch.full(tuple(shape), -1, dtype=torch.int32, device=dev)


def hip_subm(coors, shape, grid, ksize=(3, 3, 3)):
    """nbr [n, K] (device) of rpc_subm_rulebook; coors: int32 numpy [n, 4]"""
    lib = _ffi.load()
    cd = torch.from_numpy(coors).to(grid.device)
    K = ksize[0] * ksize[1] * ksize[2]
    nbr = torch.full((len(coors), K), MARK, dtype=torch.int32, device=grid.device)
    _ffi.check(lib.rpc_subm_rulebook(_ffi.ptr(cd), len(coors), _ffi.int_arr(shape), _ffi.int_arr(ksize),
                                     _ffi.ptr(grid), _ffi.ptr(nbr), _ffi.stream_of(nbr)), "rpc_subm_rulebook")
    torch.cuda.synchronize()
    return nbr


def hip_strided(coors, shape_in, geom, grid):
    """(n_out, coors_out, nbr_out, nbr_in) (device) of rpc_spconv_rulebook_count + _build; grid: the output level's
    index grid"""
    lib = _ffi.load()
    ksize, stride, pad = geom
    dev = grid.device
    K = ksize[0] * ksize[1] * ksize[2]
    n = len(coors)
    cd = torch.from_numpy(coors).to(dev)
    oshp = _ffi.int_arr(sc.out_shape(shape_in, ksize, stride, pad))
    wsb = lib.rpc_spconv_rulebook_workspace_size(n, K)
    ws = _ffi.workspace(wsb, dev)
    n_dev = torch.full((1,), MARK, dtype=torch.int32, device=dev)
    st = _ffi.stream_of(cd)
    args = (oshp, _ffi.int_arr(ksize), _ffi.int_arr(stride), _ffi.int_arr(pad), _ffi.ptr(grid))
    _ffi.check(lib.rpc_spconv_rulebook_count(_ffi.ptr(cd), n, *args, _ffi.ptr(n_dev), _ffi.ptr(ws), wsb, st),
               "rpc_spconv_rulebook_count")
    n_out = int(n_dev.item())
    assert 0 <= n_out <= n * K    # 0: no offset of any voxel lands on a whole in-range output coordinate
    # one spare row, filled with the marker: the builder writes n_out rows and no more
    coors_out = torch.full((n_out + 1, 4), MARK, dtype=torch.int32, device=dev)
    nbr_out = torch.full((n_out + 1, K), MARK, dtype=torch.int32, device=dev)
    nbr_in = torch.full((n, K), MARK, dtype=torch.int32, device=dev)
    _ffi.check(lib.rpc_spconv_rulebook_build(_ffi.ptr(cd), n, *args, n_out, _ffi.ptr(coors_out), _ffi.ptr(nbr_out),
                                             _ffi.ptr(nbr_in), _ffi.ptr(ws), st), "rpc_spconv_rulebook_build")
    torch.cuda.synchronize()
    assert (coors_out[n_out] == MARK).all() and (nbr_out[n_out] == MARK).all()
    return n_out, coors_out[:n_out], nbr_out[:n_out], nbr_in
