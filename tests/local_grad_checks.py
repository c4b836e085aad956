"""Check bodies shared by tests/test_local_grad_emu.py (the kernel sources on the fibre emulator) and
tests/test_local_grad_gpu.py (the gfx950 build): the adjoint of the local correlation (csrc/dlpd_local_grad.h) against
float64, and the differentiable LocalDockingModel against a pure-torch restatement of the reference's slices.

The expectation is computed here in numpy float64 from the adjoint's definition, by slices whose bounds are computed
arithmetically -- independently of the kernel:

    grec[p,c,X] = sum_d g[p,c,d] lig'_p[c, X - tau_p - d]        glig[p,c,x] = sum_d g[p,c,d] rec[c, x + tau_p + d]

Tolerance (derived, as in test_local_emu.py): an element is an f32 sum of at most K products in some order on both sides, so
|got - want| <= 2 (K + 1) 2^-24 sum|g v| (the sum taken in float64 here), K = W^3, times P where one gradient collects every
pose.  With a rotation the f32 sample of the rotated ligand adds the repository's parity band: 1e-4 of the largest expected
value."""
import numpy as np
import torch

from oracle import docking_oracle as orc

TOL = 1e-4
EPS = 2.0 ** -24
MODES = {"floor": 0, "trunc": 1}


def coarse(t, scale, mode):
    t = np.asarray(t, dtype=np.float64) / scale
    return (np.floor(t) if mode == "floor" else np.trunc(t)).astype(int)


def _slices(t, L):
    """rec[a] pairs with lig[b] under the signed translation t (|t_k| < L)."""
    a, b = [], []
    for v in t:
        v = int(v)
        a.append(slice(v, L) if v >= 0 else slice(0, L + v))
        b.append(slice(0, L - v) if v >= 0 else slice(-v, L))
    return (slice(None),) + tuple(a), (slice(None),) + tuple(b)


def adjoint64(rec, lig, g, tau, r):
    """One pose: rec, lig (C, L, L, L) float64 (lig already rotated), g (C, W, W, W) -> grec, glig and the sums of |terms|."""
    L = rec.shape[-1]
    grec, glig, mrec, mlig = (np.zeros_like(rec) for _ in range(4))
    for dx in range(-r, r + 1):
        for dy in range(-r, r + 1):
            for dz in range(-r, r + 1):
                t = np.asarray(tau) + np.array([dx, dy, dz])
                if (np.abs(t) >= L).any():
                    continue
                a, b = _slices(t, L)
                w = g[:, dx + r, dy + r, dz + r][:, None, None, None]
                grec[a] += w * lig[b]
                mrec[a] += np.abs(w * lig[b])
                glig[b] += w * rec[a]
                mlig[b] += np.abs(w * rec[a])
    return grec, glig, mrec, mlig


def rots(n, seed=1):
    ang = np.random.RandomState(seed).uniform(-np.pi, np.pi, size=(n, 3))
    return orc.euler_to_matrix(ang[:, 0], np.abs(ang[:, 1]), ang[:, 2])


def translations(P, L, scale, seed=0):
    """(P, 3) on the grid of scale * L points: pose 0 has components with |tau| >= L + 3 (no overlap anywhere in a window of
    radius <= 3: its gradients are exactly zero), pose 1 sits at a face (tau_x = L - 1: a window of radius >= 1 crosses it),
    the others have |tau| <= L / 4 with negative odd components at scale 2 (where floor and trunc differ)."""
    q = L // 4
    if scale == 1:
        small = [[-q, 1, -1], [1, -1, q], [-1, q, 1]]
    else:
        small = [[-(2 * q - 1), 1, -1], [3 if q >= 2 else 1, -1, 2 * q], [-1, -(2 * q - 1), 1]]
    rs = np.random.RandomState(seed)
    while len(small) < P - 2:
        small.append(list(rs.randint(-scale * q + 1, scale * q, size=3)))
    rows = [[scale * (L + 3), scale, -scale * (L + 4)], [scale * (L - 1), 0, -1]] + small[:P - 2]
    if P == 2:                                # (no room for all three kinds: the face and one well-overlapping pose)
        rows = [rows[1], small[0]]
    return np.array(rows)


def check_kernel(lib, device, L, C, r, P, scale=1, mode="trunc", shared=False, want=("rec", "lig"), rotate=False, seed=0):
    """dlpd_local_correlate_grad through ``lib.call`` against float64; the outputs start as NaN (every voxel must be
    written); two runs give the same bytes.  shared: one receptor and one ligand for all poses (stride 0, the gradient is
    the sum over the poses)."""
    g_ = torch.Generator().manual_seed(1000 * L + 10 * r + seed)
    W = 2 * r + 1
    nv = 1 if shared else P
    rec = torch.randn(nv, C, L, L, L, generator=g_)
    lig = torch.randn(nv, C, L, L, L, generator=g_)
    g = torch.randn(P, C, W, W, W, generator=g_)
    T = translations(P, L, scale, seed)
    R = torch.from_numpy(rots(P, seed=seed + L)).float().contiguous() if rotate else None
    tau = coarse(T, scale, mode)
    small = [p for p in range(P) if (np.abs(tau[p]) <= L / 4.0).all()]
    far = [p for p in range(P) if (np.abs(tau[p]) >= L + r).any()]
    face = [p for p in range(P) if tau[p][0] == L - 1]
    assert len(small) == max(P - 2, 1) and len(face) == 1 and len(far) == (1 if P > 2 else 0)
    # ---- float64 expectation, per pose
    exp = {k: np.zeros((P, C, L, L, L)) for k in ("rec", "lig", "mrec", "mlig")}
    for p in range(P):
        v = 0 if shared else p
        lp = lig[v:v + 1]
        if rotate:
            lp = orc.rotate_volume(lp, R[p:p + 1])
        exp["rec"][p], exp["lig"][p], exp["mrec"][p], exp["mlig"][p] = adjoint64(
            rec[v].numpy().astype(np.float64), lp[0].numpy().astype(np.float64), g[p].numpy().astype(np.float64), tau[p], r)
    for k in ("rec", "lig"):
        assert (exp[k][far] == 0).all()                                   # |tau| >= L + r: nothing overlaps
        body = exp[k][small].sum(axis=0) if shared else exp[k][small]
        frac = float((body != 0).mean())
        assert frac >= 0.4, ("the |tau| <= L / 4 poses must fill 40 % of the gradient", k, frac)
    # ---- the kernel
    dev = torch.device(device)
    d_rec, d_lig, d_g = rec.to(dev).contiguous(), lig.to(dev).contiguous(), g.to(dev).contiguous()
    d_T = torch.from_numpy(T).int().to(dev).contiguous()
    d_R = R.to(dev) if rotate else None
    stride = 0 if shared else C * L ** 3

    def run():
        outs = {k: torch.full((nv, C, L, L, L), float("nan"), dtype=torch.float32, device=dev) for k in want}
        args = (d_rec.data_ptr(), d_lig.data_ptr(), d_R.data_ptr() if rotate else None, d_T.data_ptr(), d_g.data_ptr(),
                outs["rec"].data_ptr() if "rec" in outs else None, outs["lig"].data_ptr() if "lig" in outs else None,
                P, C, L, r, scale, MODES[mode], float(L) / 2.0, stride, stride, _stream(dev))
        lib.call("dlpd_local_correlate_grad", *args)
        return {k: v.cpu().numpy() for k, v in outs.items()}
    got, again = run(), run()
    K = W ** 3 * (P if shared else 1)
    for k in want:
        assert got[k].tobytes() == again[k].tobytes(), "fixed summation order: the same bits run to run"
        assert not np.isnan(got[k]).any(), "every output voxel is written"
        w64 = exp[k].sum(axis=0, keepdims=True) if shared else exp[k]
        mag = exp["m" + k].sum(axis=0, keepdims=True) if shared else exp["m" + k]
        bound = 2 * (K + 1) * EPS * mag + (TOL * np.abs(w64).max() if rotate else 0.0)
        err = np.abs(got[k] - w64)
        if not rotate:
            assert (got[k][mag == 0] == 0).all()                          # no term in the box: exactly zero
        if not shared:
            assert (got[k][far] == 0).all()
        print("local_correlate_grad g%s L=%d C=%d r=%d P=%d scale %d %s%s%s: worst error %.3g of max|want|" %
              (k, L, C, r, P, scale, mode, ", shared" if shared else "", ", R" if rotate else "", err.max() / np.abs(w64).max()))
        assert (err <= bound).all(), (k, float((err - bound).max()), float(np.abs(w64).max()))


def _stream(dev):
    from deeplocalproteindocking_amd.engine import _stream as s
    return s(dev)


# ----------------------------------------------------------------------------------------------------------------------
# the model: MultiplyVolumes restated in torch (differentiable, any dtype) and the parameter gradients
# ----------------------------------------------------------------------------------------------------------------------

def multiply_torch(rec, lig, T):
    """(B, C): pair i at translation int(T[i]) -- the reference's slices (MultiplyVolumes.py:13-60), the bounds computed
    arithmetically."""
    L = rec.shape[-1]
    rows = []
    for i in range(rec.shape[0]):
        t = [int(v) for v in torch.as_tensor(T[i]).double().trunc().tolist()]
        if max(abs(v) for v in t) >= L:
            rows.append((rec[i, :, 0, 0, 0] * 0.0))
            continue
        a, b = _slices(t, L)
        rows.append((rec[i][a] * lig[i][b]).sum(dim=(1, 2, 3)))
    return torch.stack(rows)


def model_torch(representation, filt, receptor, ligand, T):
    """LocalDockingModel.forward (DockingModels.py:102-120) in plain torch, in the dtype of its arguments."""
    edge = float(receptor.shape[2])
    pairs = zip(representation(receptor), representation(ligand))
    feats = torch.cat([multiply_torch(rv, lv, T * float(rv.shape[2]) / edge) for rv, lv in pairs], dim=1)
    return filt(feats)


def check_model_gradients(label, model, receptor, ligand, T, device="cpu"):
    """out.sum().backward() through the differentiable model (kernels) against the same modules in pure torch: float64 on the
    CPU is the truth, float32 pure torch on ``device`` the yardstick (tests/accuracy_checks.py: 2x RMS, 3x max)."""
    import copy
    from accuracy_checks import yardstick
    dev = torch.device(device)
    model = model.to(dev).train()
    model.zero_grad()
    out = model(receptor.to(dev), ligand.to(dev), T.to(dev))
    out.sum().backward()
    names = [n for n, _ in model.named_parameters()]
    got = {n: p.grad for n, p in model.named_parameters()}
    assert all(got[n] is not None for n in names), [n for n in names if got[n] is None]
    grads = {}
    for dtype, where in ((torch.float64, torch.device("cpu")), (torch.float32, dev)):
        rep = copy.deepcopy(model.representation).to(device=where, dtype=dtype)
        filt = copy.deepcopy(model.filter).to(device=where, dtype=dtype)
        for m in (rep, filt):
            m.zero_grad()
        o = model_torch(rep, filt, receptor.to(device=where, dtype=dtype), ligand.to(device=where, dtype=dtype), T)
        o.sum().backward()
        grads[dtype] = {**{"representation." + n: p.grad for n, p in rep.named_parameters()},
                        **{"filter." + n: p.grad for n, p in filt.named_parameters()}}
        if dtype == torch.float64:
            out64 = o.detach()
    assert sorted(grads[torch.float64]) == sorted(names)
    for n in names:
        g64 = grads[torch.float64][n]
        assert float(g64.abs().max()) > 0, (n, "a gradient that is zero measures nothing")
        g32 = grads[torch.float32][n].detach().cpu().double()
        if torch.equal(g32, g64):          # (sums of a few exact terms, a last layer's bias: twice no error is no error)
            assert torch.equal(got[n].detach().cpu().double(), g64), (n, "float32 torch is exact here, the kernel path is not")
            continue
        yardstick("%s, d/d %s" % (label, n), got[n], g32, g64)
    return out.detach().cpu(), out64


def check_backward_split(lib, device):
    """ops.local_correlate's backward with per-pose volumes goes in batches of what the library answers to
    dlpd_local_max_poses -- here answered by a wrapper that says 5: 13 poses go as 5, 5 and 3, each batch with the bits of a
    call of its own (and the whole with the bits of the unsplit call)."""
    from deeplocalproteindocking_amd import ops

    class Limited:
        def call(self, name, *args):
            return 5 if name == "dlpd_local_max_poses" else lib.call(name, *args)

    def grads(rec, lig, T, gout, lib_):
        a, b = rec.clone().requires_grad_(), lig.clone().requires_grad_()
        ops.local_correlate(a, b, T, radius=0, lib=lib_).backward(gout)
        return a.grad.cpu().numpy(), b.grad.cpu().numpy()
    L, C, P = 8, 2, 13
    dev = torch.device(device)
    g_ = torch.Generator().manual_seed(2)
    rec, lig = torch.randn(P, C, L, L, L, generator=g_).to(dev), torch.randn(P, C, L, L, L, generator=g_).to(dev)
    T = torch.randint(-2, 3, (P, 3), generator=g_).int().to(dev)
    gout = torch.randn(P, C, 1, 1, 1, generator=g_).to(dev)
    ga, gb = grads(rec, lig, T, gout, Limited())
    wa, wb = grads(rec, lig, T, gout, lib)
    assert ga.tobytes() == wa.tobytes() and gb.tobytes() == wb.tobytes()
    for beg in (5, 10):
        sl = slice(beg, min(beg + 5, P))
        ta, tb = grads(rec[sl].contiguous(), lig[sl].contiguous(), T[sl].contiguous(), gout[sl].contiguous(), lib)
        assert ga[sl].tobytes() == ta.tobytes() and gb[sl].tobytes() == tb.tobytes()
    assert np.abs(ga).max() > 0 and np.abs(gb).max() > 0


class TwoResolutionStub(torch.nn.Module):
    """A representation for the trainer's tests: a single bias-free Conv3d, read at the input's resolution and at half of it."""

    def __init__(self, channels=3):
        super().__init__()
        self.conv = torch.nn.Conv3d(11, channels, kernel_size=3, padding=1, bias=False)
        self.channels = channels

    def get_num_outputs(self):
        return [self.channels, self.channels]

    def forward(self, x):
        y = self.conv(x)
        return [y, torch.nn.functional.avg_pool3d(y, 2)]
