"""Check bodies shared by tests/test_repr_sparse_gpu.py (the gfx950 build) and tests/test_repr_sparse_emu.py (the same kernel
sources on the fibre emulator): the tile-occupancy path of the representation stage -- ops.tile_occupancy -> ops.conv3d(occupancy=,
return_occupancy=, unwritten=) -> ops.maxpool3d_5s2(occupancy=, ...) -> dlpd_zfft_volumes_occ -- at LOPSIDED maps, one per batch
entry.  The cube inputs of tests/test_kernels_emu.py (`_blob_input`) are symmetric in x, y, z, equal in every entry, connected,
never empty and never more than three; an exchanged axis, a map read at entry 0, a neighbourhood cell left out or a dropped chunk
offset reads the same bytes there.

The supports (``supports(D)``), one batch entry each:

    cuboid_xyz   x [1, 4), y [D - 12, D - 6), z [D - 5, D): three extents, three offsets, flush with the face z = D - 1
    cuboid_yzx   the same cuboid with its axes cyclically permuted ...
    cuboid_zxy   ... twice: each of x, y, z plays each role once
    pieces       one voxel (7, 8, 3) -- last of its cell in x and z, first in y -- and a plate on x = D - 1 (z < D / 2)
    corner       one voxel (D - 1, 0, D - 1)
    empty        zero everywhere
    full         non-zero everywhere
    subnormal    one 1e-40 alone in its cell (5, 6, 2), and a 2 x 2 x 2 block far away

Comparisons are bit equality (torch.equal) or the project's yardstick (accuracy_checks.yardstick: torch's float32 conv3d is
X32, its float64 one X64; RMS_MARGIN, MAX_MARGIN) -- there is no tolerance of this file's own.  Every case asserts what it
claims about its inputs (``claims``): entries pairwise different, which have empty cells, which have convolution blocks with an
all-empty neighbourhood, one all empty, one all full.  Nothing here reads the reference tree."""
import os
import tempfile

import numpy as np
import torch
import torch.nn.functional as F

import accuracy_checks as acc

NAMES = ("cuboid_xyz", "cuboid_yzx", "cuboid_zxy", "pieces", "corner", "empty", "full", "subnormal")
CIN = 11                                   # not a multiple of the kernel's 8-channel chunk
WIDTHS = (16, 16, 48, 32)                  # conv k5 + ReLU -> conv k3 -> pool -> conv k5 (a 32-group plus a 16-group) -> conv k3
LAYERS = (("conv", 0, 5, True), ("conv", 1, 3, False), ("pool",), ("conv", 2, 5, False), ("conv", 3, 3, False))
SUBNORMAL = 1e-40


# ----------------------------------------------------------------------------------------------------------------------
# inputs and host references
# ----------------------------------------------------------------------------------------------------------------------

def supports(D, cin=CIN, seed=3, which=None):
    """-> (x (B, cin, D, D, D) float32 on the host, names): randn in all channels on the support of each entry, zero elsewhere."""
    assert D >= 13
    g = torch.Generator().manual_seed(seed + D)
    a, b, c = (1, 4), (D - 12, D - 6), (D - 5, D)
    masks = {}
    for name, (rx, ry, rz) in (("cuboid_xyz", (a, b, c)), ("cuboid_yzx", (c, a, b)), ("cuboid_zxy", (b, c, a))):
        m = torch.zeros(D, D, D, dtype=torch.bool)
        m[rx[0]:rx[1], ry[0]:ry[1], rz[0]:rz[1]] = True
        masks[name] = m
    m = torch.zeros(D, D, D, dtype=torch.bool)
    m[7, 8, 3] = True                                              # (4 i + 3, 4 j, 4 k + 3)
    m[D - 1, :, :D // 2] = True
    masks["pieces"] = m
    m = torch.zeros(D, D, D, dtype=torch.bool)
    m[D - 1, 0, D - 1] = True
    masks["corner"] = m
    masks["empty"] = torch.zeros(D, D, D, dtype=torch.bool)
    masks["full"] = torch.ones(D, D, D, dtype=torch.bool)
    m = torch.zeros(D, D, D, dtype=torch.bool)
    m[D - 3:D - 1, D - 3:D - 1, D - 3:D - 1] = True
    masks["subnormal"] = m
    names = [n for n in NAMES if which is None or n in which]
    x = torch.zeros(len(names), cin, D, D, D)
    for i, n in enumerate(NAMES):                                   # (every entry draws the same numbers whatever ``which`` is)
        v = torch.randn(cin, D, D, D, generator=g)
        v[v == 0] = 1.0
        if n in names:
            x[names.index(n)] = v * masks[n]
    if "subnormal" in names:
        x[names.index("subnormal"), cin - 1, 5, 6, 2] = SUBNORMAL
        assert 0 < float(x[names.index("subnormal"), cin - 1, 5, 6, 2]) < 1.1754944e-38
    return x, names


def _NanEmpty():
    """The NaN-prefill of tests/test_kernels_emu.py: inside the block ``torch.empty`` hands out NaN-filled buffers."""
    from test_kernels_emu import _NanEmpty as nan_empty
    return nan_empty()


def _cells(occ, D):
    """uint8 (B, nc, nc, nc) cell map -> bool (B, 1, D, D, D) voxel mask"""
    m = occ.bool().repeat_interleave(4, 1).repeat_interleave(4, 2).repeat_interleave(4, 3)[:, :D, :D, :D]
    return m[:, None]


def host_map(x):
    """The reference map: pad to a multiple of 4, ``!= 0`` by torch on the host, any over the channels and each 4^3 cell."""
    x = x.detach().cpu()
    B, D = x.shape[0], x.shape[2]
    nc = (D + 3) // 4
    p = 4 * nc - D
    nz = (F.pad(x, (0, p, 0, p, 0, p)) != 0).any(1)
    return nz.reshape(B, nc, 4, nc, 4, nc, 4).permute(0, 1, 3, 5, 2, 4, 6).reshape(B, nc, nc, nc, 64).any(-1).to(torch.uint8)


def conv_skipped_blocks(occ):
    """(B,) number of 4 x 4 x 16 convolution blocks whose neighbourhood -- 3 x 3 tile columns, the block's four z cells widened
    by one either way -- holds no occupied cell of ``occ`` (B, nc, nc, nc): the blocks the kernel neither stages nor computes."""
    occ = occ.cpu().float()
    B, nc = occ.shape[0], occ.shape[1]
    o = F.pad(occ, (1, 8, 1, 1, 1, 1))
    cnt = torch.zeros(B, dtype=torch.long)
    for bz in range((nc + 3) // 4):
        col = o[:, :, :, 4 * bz:4 * bz + 6].amax(3)                # z cells 4 bz - 1 .. 4 bz + 4
        cnt += (F.max_pool2d(col[:, None], 3, 1)[:, 0] == 0).sum((1, 2))
    return cnt


def pool_skipped_tiles(occ, D):
    """(B,) number of 4 x 4 x 20 output tiles of MaxPool(5, 2, 2) whose 11 x 11 x 43 input region (cut at the box) lies in empty
    cells of ``occ``."""
    occ = occ.cpu()
    B = occ.shape[0]
    Do = (D - 1) // 2 + 1
    cnt = torch.zeros(B, dtype=torch.long)

    def cells(o0, n):
        return max(2 * o0 - 2, 0) >> 2, (min(2 * o0 - 2 + n - 1, D - 1) >> 2) + 1
    for ox in range(0, Do, 4):
        for oy in range(0, Do, 4):
            for oz in range(0, Do, 20):
                (x0, x1), (y0, y1), (z0, z1) = cells(ox, 11), cells(oy, 11), cells(oz, 43)
                cnt += (occ[:, x0:x1, y0:y1, z0:z1].reshape(B, -1).amax(1) == 0).long()
    return cnt


def claims(x, names, D):
    """What a case says about its own inputs; -> (host map, skipped convolution blocks per entry)."""
    want = host_map(x)
    B, nc = len(names), (D + 3) // 4
    assert want.shape == (B, nc, nc, nc)
    for i in range(B):
        for j in range(i):
            assert not torch.equal(x[i], x[j]) and not torch.equal(want[i], want[j]), (names[i], names[j])
    skipped = conv_skipped_blocks(want)
    nblk = nc * nc * ((nc + 3) // 4)
    for i, n in enumerate(names):
        cells = int(want[i].sum())
        if n == "empty":
            assert cells == 0 and not x[i].any() and int(skipped[i]) == nblk
        elif n == "full":
            assert cells == nc ** 3 and bool((x[i] != 0).all()) and int(skipped[i]) == 0
        else:
            assert 0 < cells < nc ** 3 and 0 < int(skipped[i]) < nblk, (n, cells, int(skipped[i]))
    if D % 4 and B == len(NAMES):                                   # partial last cells are occupied somewhere (one voxel at D = 21 / 13 / 37)
        assert want[:, -1].any() and want[:, :, -1].any() and want[:, :, :, -1].any()
    if "subnormal" in names:
        assert want[names.index("subnormal"), 1, 1, 0] == 1         # the reference predicate keeps the subnormal
    return want, skipped


def weights(seed=5):
    g = torch.Generator().manual_seed(seed)
    cins = (CIN,) + WIDTHS[:-1]
    return [torch.randn(WIDTHS[i], cins[i], L[2], L[2], L[2], generator=g) * 0.1 for i, L in
            enumerate(l for l in LAYERS if l[0] == "conv")]


def chain(lib, x, w, occ=None, unwritten=False, depth=len(LAYERS)):
    """conv k5 + ReLU -> conv k3 -> MaxPool(5, 2, 2) -> conv k5 -> conv k3 (the first ``depth`` layers); -> [(y, map or None)]
    per layer.  occ: the map of x."""
    from deeplocalproteindocking_amd import ops
    out = []
    for layer in LAYERS[:depth]:
        if layer[0] == "conv":
            if occ is None:
                x = ops.conv3d(x, w[layer[1]], relu=layer[3], lib=lib, precision="split_bf16")
            else:
                x, occ = ops.conv3d(x, w[layer[1]], relu=layer[3], lib=lib, precision="split_bf16", occupancy=occ,
                                    return_occupancy=True, unwritten=unwritten)
        elif occ is None:
            x = ops.maxpool3d_5s2(x, lib=lib)
        else:
            x, occ = ops.maxpool3d_5s2(x, lib=lib, occupancy=occ, return_occupancy=True, unwritten=unwritten)
        out.append((x, occ))
    return out


class _Case(object):
    pass


_CASES = {}


def case(lib, device, D, which=None, depth=len(LAYERS)):
    """The supports, the dense chain and the chain with maps of one box: made once, shared by the checks, never changed."""
    key = (id(lib), str(device), D, which, depth)
    if key not in _CASES:
        c = _Case()
        c.D, c.Dp, c.depth = D, (D - 1) // 2 + 1, depth
        c.xh, c.names = supports(D, which=which)
        c.want0, c.skipped0 = claims(c.xh, c.names, D)
        c.x = c.xh.to(device)
        c.w = [t.to(device) for t in weights()]
        from deeplocalproteindocking_amd import ops
        c.occ0 = ops.tile_occupancy(c.x, lib=lib)
        c.dense = [y for y, _ in chain(lib, c.x, c.w, depth=depth)]
        c.maps = chain(lib, c.x, c.w, c.occ0, depth=depth)
        c.sizes = [D, D, c.Dp, c.Dp, c.Dp]
        _CASES[key] = c
    return _CASES[key]


def release_cases():
    """Drop the shared cases (a test module's teardown: on the device they hold every layer of every box)."""
    _CASES.clear()


def _expand(u, m, D):
    """(tensor, map) -> the tensor it stands for: zeros where the map is 0"""
    return torch.where(_cells(m, D).expand_as(u), u, torch.zeros_like(u))


# ----------------------------------------------------------------------------------------------------------------------
# A: the map
# ----------------------------------------------------------------------------------------------------------------------

def check_map(lib, device, D):
    """ops.tile_occupancy against the host map, exactly and per entry: partial last cells, the all-empty entry, the subnormal."""
    from deeplocalproteindocking_amd import ops
    x, names = supports(D)
    want, _ = claims(x, names, D)
    got = ops.tile_occupancy(x.to(device), lib=lib).cpu()
    assert got.shape == want.shape and got.dtype == torch.uint8
    for b, n in enumerate(names):
        assert torch.equal(got[b], want[b]), (n, (got[b] != want[b]).nonzero()[:5].tolist())
    # a batch of one: the same map as the entry has inside the batch
    for n in ("cuboid_zxy", "empty"):
        b = names.index(n)
        assert torch.equal(ops.tile_occupancy(x[b:b + 1].to(device), lib=lib).cpu()[0], want[b]), n


# ----------------------------------------------------------------------------------------------------------------------
# B: skipping changes no bit
# ----------------------------------------------------------------------------------------------------------------------

def check_skipping_changes_no_bit(lib, device, D, which=None, depth=len(LAYERS)):
    c = case(lib, device, D, which, depth)
    assert torch.equal(c.occ0.cpu(), c.want0)
    for k, (d, (y, m)) in enumerate(zip(c.dense, c.maps)):
        assert torch.equal(y, d), ("layer", k, [c.names[b] for b in range(len(c.names)) if not torch.equal(y[b], d[b])])
        want = host_map(d)
        for b, n in enumerate(c.names):
            assert torch.equal(m[b].cpu(), want[b]), ("layer", k, n)
        if "empty" in c.names:
            e = c.names.index("empty")
            assert not y[e].any() and not m[e].any()
        if "full" in c.names:
            assert m[c.names.index("full")].all()
    assert float(c.dense[0].min()) == 0.0 < float(c.dense[0].max())                       # (ReLU)
    assert depth < 2 or float(c.dense[1].min()) < 0.0 < float(c.dense[1].max())           # the pooling's input has both signs


# ----------------------------------------------------------------------------------------------------------------------
# C: unwritten activations
# ----------------------------------------------------------------------------------------------------------------------

def _unwritten_agrees(c, uw, occ_first):
    """``uw`` (the chain run with unwritten=True into NaN-filled buffers) against the dense chain and the maps of B."""
    occ_in, nan_entries = occ_first.cpu(), 0
    for k, (d, (y, m), (u, n)) in enumerate(zip(c.dense, c.maps, uw)):
        Dk = c.sizes[k]
        assert torch.equal(m, n), ("layer", k)
        live = _cells(m, Dk).expand_as(d)
        assert torch.equal(d[live], u[live]) and not torch.isnan(u[live]).any(), ("layer", k)
        assert bool((d[~live] == 0).all()), ("layer", k)
        skipped = pool_skipped_tiles(occ_in, c.D) if LAYERS[k][0] == "pool" else conv_skipped_blocks(occ_in)
        for b, name in enumerate(c.names):                          # NaNs are left exactly in the entries with skipped blocks
            assert bool(torch.isnan(u[b]).any()) == bool(skipped[b] > 0), ("layer", k, name, int(skipped[b]))
            nan_entries += int(skipped[b] > 0)
        for b in range(len(c.names)):
            if not occ_in[b].any():
                assert torch.isnan(u[b]).all(), ("layer", k, c.names[b])         # an all-empty map: nothing was written
        occ_in = m.cpu()
    return nan_entries


def unwritten_chain(c, lib):
    """The chain with unwritten activations into NaN-filled buffers (made once per case)."""
    if getattr(c, "uw", None) is None:
        with _NanEmpty():
            c.uw = chain(lib, c.x, c.w, c.occ0, unwritten=True, depth=c.depth)
    return c.uw


def check_unwritten(lib, device, D, which=None, depth=len(LAYERS)):
    c = case(lib, device, D, which, depth)
    n = _unwritten_agrees(c, unwritten_chain(c, lib), c.occ0)
    assert n >= depth and int(c.skipped0.sum()) > 0                  # blocks were skipped at every layer


# ----------------------------------------------------------------------------------------------------------------------
# D: covering maps
# ----------------------------------------------------------------------------------------------------------------------

def check_covering_maps(lib, device, D, which=None, seed=23):
    """A map that covers the non-zero cells -- the exact one OR-ed with a fifth of the empty cells, then all ones -- gives
    the same bits and hands on the same maps as the exact one; so does the unwritten mode (x is zero in the extra cells)."""
    c = case(lib, device, D, which)
    exact = c.occ0.cpu()
    g = torch.Generator().manual_seed(seed)
    extra = ((torch.rand(exact.shape, generator=g) < 0.2) & (exact == 0)).to(torch.uint8)
    some = exact | extra
    for b, n in enumerate(c.names):
        if n != "full":
            assert extra[b].any() and int(some[b].sum()) < some[b].numel(), n
    assert int(conv_skipped_blocks(some).sum()) < int(c.skipped0.sum())          # the extra cells wake blocks up
    for cover in (some, torch.ones_like(exact)):
        got = chain(lib, c.x, c.w, cover.to(device))
        for k, ((y, m), (y0, m0)) in enumerate(zip(got, c.maps)):
            assert torch.equal(y, y0) and torch.equal(m, m0), ("layer", k, int(cover.sum()))
    assert not torch.isnan(c.x).any() and not c.xh[_cells(extra, D).expand_as(c.xh)].any()
    with _NanEmpty():
        uw = chain(lib, c.x, c.w, some.to(device), unwritten=True)
    _unwritten_agrees(c, uw, some)


# ----------------------------------------------------------------------------------------------------------------------
# E: truth
# ----------------------------------------------------------------------------------------------------------------------

def check_truth(lib, device, D, which=None, depth=len(LAYERS)):
    """Every convolution of the chain with maps, fed the kernel's own previous output, under the yardstick against torch's
    float32 (X32) and float64 (X64) conv3d of that input; the pooling equal to torch's."""
    c = case(lib, device, D, which, depth)
    uw = unwritten_chain(c, lib)
    prev, rows = c.xh, []
    for k, layer in enumerate(LAYERS[:depth]):
        got = _expand(uw[k][0], uw[k][1], c.sizes[k]).cpu()
        assert not torch.isnan(got).any()
        if layer[0] == "pool":
            assert torch.equal(got, F.max_pool3d(prev, kernel_size=5, stride=2, padding=2)), ("layer", k)
        else:
            w = c.w[layer[1]].cpu()
            x32 = F.conv3d(prev, w, padding=layer[2] // 2)
            x64 = F.conv3d(prev.double(), w.double(), padding=layer[2] // 2)
            if layer[3]:
                x32, x64 = torch.relu(x32), torch.relu(x64)
            rows.append(acc.yardstick("sparse conv3d layer %d, %d -> %d, k %d, D %d, %d entries" %
                                      (k, w.shape[1], w.shape[0], layer[2], c.sizes[k], len(c.names)), got, x32, x64))
        prev = c.dense[k].cpu()
    return rows


def check_pool_windows(lib, device, D, C=CIN):
    """MaxPool(5, 2, 2) with maps on supports that are NEGATIVE wherever they are occupied, against torch's, written and
    unwritten.  The three kinds of window are present: inside occupied voxels (a negative maximum); over occupied voxels and
    empty cells (0 from a cell nobody read); at the box border over -inf padding and empty cells only."""
    from deeplocalproteindocking_amd import ops
    x, names = supports(D, cin=C)
    x = torch.where(x != 0, -x.abs() - 0.3, x)
    occ_h = host_map(x)
    claims(x, names, D)
    want = F.max_pool3d(x, kernel_size=5, stride=2, padding=2)
    Do = want.shape[2]
    # the kinds of window, from the inputs alone
    sup = F.max_pool3d((x != 0).any(1, keepdim=True).float(), 5, 2, 2) > 0                    # holds an occupied voxel
    hole = F.max_pool3d((~_cells(occ_h, D)).float(), 5, 2, 2) > 0                             # holds a voxel of an empty cell
    stray = F.max_pool3d(((x[:, :1] == 0) & _cells(occ_h, D)).float(), 5, 2, 2) > 0           # holds a ZERO of an occupied cell
    o = torch.arange(Do)
    edge1 = (2 * o - 2 < 0) | (2 * o + 2 > D - 1)
    edge = (edge1[:, None, None] | edge1[None, :, None] | edge1[None, None, :])[None, None]
    partial = torch.tensor([n not in ("empty", "full") for n in names])[:, None, None, None, None]
    assert bool((want < 0).any())                                                             # a negative maximum
    # ... a 0 whose every zero voxel lies in an empty cell: over occupied voxels and empty cells; over padding and empty cells only
    assert bool(((want[:, :1] == 0) & sup & hole & ~stray & partial).any())
    assert bool(((want[:, :1] == 0) & ~sup & hole & ~stray & edge & partial).any())
    xd, occ = x.to(device), ops.tile_occupancy(x.to(device), lib=lib)
    assert torch.equal(occ.cpu(), occ_h)
    want_map = host_map(want)
    y0 = ops.maxpool3d_5s2(xd, lib=lib)
    y1, m1 = ops.maxpool3d_5s2(xd, lib=lib, occupancy=occ, return_occupancy=True)
    with _NanEmpty():
        y2, m2 = ops.maxpool3d_5s2(xd, lib=lib, occupancy=occ, return_occupancy=True, unwritten=True)
    assert torch.equal(y0.cpu(), want) and torch.equal(y1.cpu(), want)
    assert torch.equal(m1.cpu(), want_map) and torch.equal(m2.cpu(), want_map)
    assert torch.equal(_expand(y2, m2, Do).cpu(), want) and torch.isnan(y2[names.index("empty")]).all()
    skipped = pool_skipped_tiles(occ_h, D)
    for b, n in enumerate(names):
        assert bool(torch.isnan(y2[b]).any()) == bool(skipped[b] > 0), n


# ----------------------------------------------------------------------------------------------------------------------
# F: the consumer
# ----------------------------------------------------------------------------------------------------------------------

def check_consumer(lib, device, L, C, which=None):
    """dlpd_zfft_volumes_occ on an unwritten tensor plus map against dlpd_zfft_into on the dense tensor, in a NaN-filled
    workspace.  The contract of include/dlpd.h: an x-plane without an occupied cell -- every plane of an all-empty entry --
    is written as zeros without a transform (skip_empty = 0), or not written at all (skip_empty = 1; there the consumer goes
    by the pencil map, the maps' OR over z, so the pencils that map marks must hold the dense spectra)."""
    from deeplocalproteindocking_amd import ops
    from deeplocalproteindocking_amd._lib import get_lib
    call = (lib or get_lib()).call
    xh, names = supports(L, which=which)
    claims(xh, names, L)
    g = torch.Generator().manual_seed(31)
    w = (torch.randn(C, CIN, 5, 5, 5, generator=g) * 0.1).to(device)
    x = xh.to(device)
    occ0 = ops.tile_occupancy(x, lib=lib)
    with _NanEmpty():
        u1, n1 = ops.conv3d(x, w, lib=lib, precision="split_bf16", occupancy=occ0, return_occupancy=True, unwritten=True)
    d1 = ops.conv3d(x, w, lib=lib, precision="split_bf16")
    live = _cells(n1, L).expand_as(d1)
    assert torch.equal(n1.cpu(), host_map(d1)) and torch.equal(u1[live], d1[live]) and bool((d1[~live] == 0).all())
    B, NZ = len(names), L + 1
    e = names.index("empty")
    assert torch.isnan(u1[e]).all() and not n1[e].any() and any(bool(torch.isnan(u1[b]).any()) for b in range(B) if b != e)
    st = torch.cuda.current_stream(device).cuda_stream if str(device) != "cpu" else 0
    A_d = torch.zeros(B, C + 1, NZ, L, L, 2, device=device)
    A_u = torch.full((B, C + 1, NZ, L, L, 2), float("nan"), device=device)
    A_s = torch.full((B, C + 1, NZ, L, L, 2), float("nan"), device=device)
    call("dlpd_zfft_into", d1.data_ptr(), 0, A_d.data_ptr(), B, C, C + 1, 0, L, C * L ** 3, 0, 0.0, st)
    call("dlpd_zfft_volumes_occ", u1.data_ptr(), n1.data_ptr(), A_u.data_ptr(), B, C, C + 1, 0, L, C * L ** 3, 0, st)
    call("dlpd_zfft_volumes_occ", u1.data_ptr(), n1.data_ptr(), A_s.data_ptr(), B, C, C + 1, 0, L, C * L ** 3, 1, st)
    for b, n in enumerate(names):
        assert torch.equal(A_d[b, :C], A_u[b, :C]), n
    assert torch.isnan(A_u[:, C]).all() and torch.isnan(A_s[:, C]).all()         # the channel the call does not own
    assert bool((A_u[e, :C] == 0).all()) and bool((A_d[e, :C] == 0).all())      # zeros, written without a transform
    assert torch.isnan(A_s[e]).all()                                             # not written at all
    pencil = n1.cpu().bool().any(3).repeat_interleave(4, 1).repeat_interleave(4, 2)[:, :L, :L]       # (B, x, y)
    plane = pencil.any(2)[:, None, None, :, None, None].expand(B, C, NZ, L, L, 2)                    # x-planes with an occupied cell
    pencil = pencil[:, None, None, :, :, None].expand(B, C, NZ, L, L, 2)
    A_s, A_d = A_s[:, :C].cpu(), A_d[:, :C].cpu()
    assert torch.equal(A_s[pencil], A_d[pencil]) and torch.isnan(A_s[~plane]).all()
    assert any(0 < int(plane[b].sum()) < plane[b].numel() for b in range(B))                         # an entry with both kinds of plane
    assert 0 < int(pencil.sum()) < pencil.numel() and ("full" not in names or bool(pencil[names.index("full")].all()))


# ----------------------------------------------------------------------------------------------------------------------
# G: the plugin
# ----------------------------------------------------------------------------------------------------------------------

def plugin(lib, device, seed=41):
    from deeplocalproteindocking_amd.Models.ProteinRepresentationModels import E3MultiResRepr4x4
    rep = E3MultiResRepr4x4(multiplier=8)
    g = torch.Generator().manual_seed(seed)
    for p in rep.parameters():
        fan = p.shape[1] * p.shape[2] ** 3
        p.data = torch.randn(p.shape, generator=g) * (2.0 / fan) ** 0.5
    rep = rep.to(device).eval()
    rep.hip_lib = lib if str(device) == "cpu" else None
    assert rep.use_hip_conv and rep.supports_unwritten_outputs
    return rep


def _plugin_agrees(rep, dense_in, sparse_in, names):
    """The plugin inside outputs_with_maps() (on ``sparse_in``), with use_tile_occupancy = False and plain (on ``dense_in``)."""
    with torch.no_grad():
        rep.use_tile_occupancy = False
        dense = rep(dense_in)
        rep.use_tile_occupancy = True
        plain = rep(dense_in)
        with _NanEmpty(), rep.outputs_with_maps():
            uw = rep(sparse_in)
    assert len(dense) == len(plain) == len(uw) == 2 and dense[1].shape[2] == (dense[0].shape[2] - 1) // 2 + 1
    nan_left = False
    for r, (d, p, u) in enumerate(zip(dense, plain, uw)):
        assert getattr(d, "dlpd_occupancy", None) is None
        want = host_map(d)
        assert torch.equal(p, d), ("resolution", r)
        for b, n in enumerate(names):
            assert torch.equal(p.dlpd_occupancy[b].cpu(), want[b]) and torch.equal(u.dlpd_occupancy[b].cpu(), want[b]), (r, n)
        live = _cells(u.dlpd_occupancy, d.shape[2]).expand_as(d)
        assert torch.equal(u[live], d[live]) and bool((d[~live] == 0).all()), ("resolution", r)
        nan_left |= bool(torch.isnan(u).any())
        assert d.abs().max() > 0
    assert nan_left
    return dense, uw


def check_plugin(lib, device, D, which=None):
    rep = plugin(lib, device)
    xh, names = supports(D, which=which)
    claims(xh, names, D)
    x = xh.to(device)
    dense, uw = _plugin_agrees(rep, x, x, names)
    if "empty" in names:
        e = names.index("empty")
        assert all(torch.isnan(u[e]).all() and not u.dlpd_occupancy[e].any() and not d[e].any() for d, u in zip(dense, uw))


def check_outputs_with_maps_is_per_thread(lib, device, D=13):
    """``outputs_with_maps()`` entered on one thread leaves a forward of the SAME module on another thread dense (a sweep
    prepares the next receptor on a second host thread while the search holds the context open), and still holds on its own
    thread afterwards.  One worker, started and joined inside the context: nothing here depends on timing."""
    import threading
    rep = plugin(lib, device)
    xh, names = supports(D, which=("corner",))                     # (one voxel: most tiles stay empty, so NaNs can be left)
    x = xh.to(device)
    with torch.no_grad():
        before = rep(x)
    got = {}

    def worker():                                                  # (grad mode is per thread too: a new thread starts with it on)
        try:
            with torch.no_grad(), _NanEmpty():
                got["volumes"] = rep(x)
        except BaseException as e:
            got["error"] = e
    with rep.outputs_with_maps():
        t = threading.Thread(target=worker)
        t.start()
        t.join()
        with torch.no_grad(), _NanEmpty():
            uw = rep(x)
    assert "error" not in got, got.get("error")
    assert len(got["volumes"]) == len(before) == len(uw) == 2
    for b, w in zip(before, got["volumes"]):
        assert torch.equal(w, b) and not bool(torch.isnan(w).any())
    nan_left = False
    for d, u in zip(before, uw):                                   # the main thread is still inside: maps, NaNs outside them
        assert torch.equal(u.dlpd_occupancy.cpu(), host_map(d))
        live = _cells(u.dlpd_occupancy, d.shape[2]).expand_as(d)
        assert torch.equal(u[live], d[live]) and bool((d[~live] == 0).all())
        nan_left |= bool(torch.isnan(u).any())
    assert nan_left


def check_plugin_on_projected_protein(lib, device, L, res):
    """A CoordsBackend.project(cells=True) volume -- unwritten outside the cells the atoms' windows reach, with a map that
    COVERS its non-zero cells -- of a synthetic protein under three oblique rotations, one of which swings most atoms out of
    the box, through the plugin against the dense projection through the dense plugin."""
    from deeplocalproteindocking_amd.Utils.FullAtom import CoordsBackend
    from synth_pdb import write_protein_like_pdb
    be = CoordsBackend(lib=lib if str(device) == "cpu" else None)
    with tempfile.TemporaryDirectory(prefix="dlpd_repr_sparse_") as tmp:
        f = os.path.join(tmp, "p.pdb")
        write_protein_like_pdb(f, 24, seed=7, nchains=1, extras=False)
        coords, _, rn, _, an, nat = be.pdb2coords([f])
    typed, counts, offs = be.assign_types(coords, rn, an, nat)
    n = int(be.last_num_typed[0])
    lo, hi = be.get_bbox(typed, be.last_num_typed)
    half = L * res / 2.0
    # the protein sits off the rotation centre, towards the box edge x = y
    off = torch.tensor([[0.36 * L * res, 0.36 * L * res, 0.0]], dtype=torch.double)
    typed = be.translate(typed, off - (lo + hi) * 0.5, be.last_num_typed)

    def rot(axis, deg):
        return acc.axis_angle(np.asarray(axis, dtype=np.float64), np.deg2rad(deg))
    R = np.stack([rot((1.0, -1.0, 0.3), 35.0), rot((-2.0, 1.0, 0.5), 33.0), rot((0.2, -0.1, 1.0), 43.0)])
    assert all(np.abs(r).min() > 1e-3 for r in R)                   # oblique: no axis stays an axis
    p = typed[0, :3 * n].reshape(n, 3).numpy()
    inside = [float(((q >= -half) & (q < half)).all(1).mean()) for q in (p @ r.T for r in R)]
    assert inside[0] > 0.6 and inside[1] > 0.6 and inside[2] < 0.4, inside
    Rt = torch.from_numpy(R).float().to(device)
    centre = torch.full((1, 3), half, dtype=torch.double)
    dense_in = be.project(typed, counts, offs, L, res, device, R=Rt, shift=centre)
    with _NanEmpty():
        sparse_in = be.project(typed, counts, offs, L, res, device, R=Rt, shift=centre, cells=True)
    occ = sparse_in.dlpd_occupancy
    exact = host_map(dense_in)
    assert sparse_in.dlpd_unwritten and bool((occ.cpu() >= exact).all()) and bool(torch.isnan(sparse_in).any())
    assert all(0 < int(occ[b].sum()) < occ[b].numel() for b in range(3)) and int(occ[2].sum()) < int(occ[0].sum())
    assert len({occ[b].cpu().numpy().tobytes() for b in range(3)}) == 3
    rep = plugin(lib, device)
    _plugin_agrees(rep, dense_in, sparse_in, ["rotation %d" % b for b in range(3)])


# ----------------------------------------------------------------------------------------------------------------------
# H: the pooling's chunk loop
# ----------------------------------------------------------------------------------------------------------------------

def check_pool_many_volumes(lib, device, nvol=8 * 65535 + 9):
    """More volumes than a grid's z extent holds blocks of eight: the (nvol, 1) form, several launches."""
    from deeplocalproteindocking_amd import ops
    assert (nvol + 7) // 8 > 65535
    g = torch.Generator().manual_seed(51)
    x = torch.randn(nvol, 1, 2, 2, 2, generator=g)
    want = F.max_pool3d(x, kernel_size=5, stride=2, padding=2)
    y = ops.maxpool3d_5s2(x.to(device), lib=lib)
    assert y.shape == want.shape == (nvol, 1, 1, 1, 1) and torch.equal(y.cpu(), want)
    assert not torch.equal(want[:9], want[65535:65535 + 9])


def check_pool_chunked_maps(lib, device, B=65535 + 6, D=5):
    """The maps form over two launches: the second starts dlpd_conv3d_tile_occupancy_bytes(b0, D) into both maps.  Per-entry
    random supports, about one entry in three all empty."""
    from deeplocalproteindocking_amd import ops
    from deeplocalproteindocking_amd._lib import get_lib
    call = (lib or get_lib()).call
    per = 65535
    assert per < B < 2 * per
    nc, Do = (D + 3) // 4, (D - 1) // 2 + 1
    g = torch.Generator().manual_seed(53)
    cells = (torch.rand(B, nc, nc, nc, generator=g) < 0.4) & (torch.rand(B, 1, 1, 1, generator=g) > 1.0 / 3.0)
    for j in range(B - per):                                        # the second launch's entries and the ones a dropped offset
        cells[j], cells[per + j] = False, False                     # would read instead: empty where the other is not
        cells[per + j if j % 2 else j, j % nc, 0, 1] = True
    x = torch.randn(B, 1, D, D, D, generator=g) - 0.3
    x[1::2] = -x[1::2].abs() - 0.3                                  # (every other entry negative wherever it is occupied)
    x = x * _cells(cells.to(torch.uint8), D)
    occ_h = host_map(x)
    assert torch.equal(occ_h, cells.to(torch.uint8))
    none = ~cells.reshape(B, -1).any(1)
    assert 0.3 < float(none.float().mean()) < 0.45
    assert all(bool(none[j]) != bool(none[per + j]) for j in range(B - per)) and none[per:].any() and not none[per:].all()
    assert call("dlpd_conv3d_tile_occupancy_bytes", per, D) == per * nc ** 3
    want = F.max_pool3d(x, kernel_size=5, stride=2, padding=2)
    want_map = host_map(want)
    assert bool((want < 0).any()) and bool((want > 0).any())
    xd, occ = x.to(device), occ_h.to(device)                       # (the host map: the map kernel takes one block layer per entry)
    y1, m1 = ops.maxpool3d_5s2(xd, lib=lib, occupancy=occ, return_occupancy=True)
    assert torch.equal(y1.cpu(), want) and torch.equal(m1.cpu(), want_map)
    with _NanEmpty():
        y2, m2 = ops.maxpool3d_5s2(xd, lib=lib, occupancy=occ, return_occupancy=True, unwritten=True)
    assert torch.equal(m2.cpu(), want_map)
    y2 = y2.cpu()
    assert torch.equal(torch.isnan(y2).reshape(B, -1).any(1), none) and torch.equal(torch.isnan(y2).reshape(B, -1).all(1), none)
    assert torch.equal(torch.where(torch.isnan(y2), torch.zeros_like(y2), y2), want)
