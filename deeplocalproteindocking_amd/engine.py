"""Host-side driver of the HIP pipeline: owns the device workspaces (as torch tensors) and
enqueues the C-ABI calls of include/dlpd.h on torch's current stream.

It mirrors the body of the reference's hot loop, src/Docker/Docker.py:211-236 (rotate ligand
volumes, clash correlation + threshold, GlobalDockingModel.forward, mask multiply, update_top)
for a single-resolution representation, without any host synchronisation inside the loop.
torch is plumbing only (memory + streams); all arithmetic is in libdlpd.so.
"""
import numpy as np
import torch

from ._lib import get_lib


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _stream(device):
    if device.type == "cuda":
        return torch.cuda.current_stream(device).cuda_stream
    return 0


def key_to_float(key):
    """Inverse of the order-preserving float key used in the device top-K list."""
    key = np.asarray(key, dtype=np.uint32)
    neg = (key & np.uint32(0x80000000)) == 0
    bits = np.where(neg, ~key, key & np.uint32(0x7FFFFFFF)).astype(np.uint32)
    return bits.view(np.float32)


class DeviceTopList:
    """Device-resident running top list: the state Docker.update_top keeps in ``self.top_list``
    (Docker.py:100-105), plus the per-rotation pick buffers (Docker.py:89-98)."""

    def __init__(self, K, batch, device, lib, exclusion=0):
        self.K, self.batch, self.device, self.lib = int(K), int(batch), torch.device(device), lib
        dev = self.device
        # exclusion radius in voxels (include/dlpd.h, dlpd_topk_suppress; build-defined, 0 = the reference): settable between
        # selects; Vs, the suppressed copy of a batch's scores, is made at the first select that needs it
        self.exclusion = exclusion
        self._Vs = None
        # distance restraints (include/dlpd.h, dlpd_topk_restrain; build-defined, None = the reference): set_restraints
        self.restraints = None
        self._rst = None
        self.cand_score = torch.empty(batch, self.K, dtype=torch.float32, device=dev)
        self.cand_idx = torch.empty(batch, self.K, dtype=torch.int32, device=dev)
        self.ws = torch.empty(lib.call("dlpd_topk_workspace_bytes", batch, self.K), dtype=torch.uint8, device=dev)
        self.glist = torch.zeros(lib.call("dlpd_topk_glist_bytes", self.K) // 8, dtype=torch.int64, device=dev)
        # candidate filter of the scoring kernel (include/dlpd.h, dlpd_topk_merge_tau): key of the list's K-th score
        # once the list is full and that score negative, else 0
        self.tau = torch.zeros(4, dtype=torch.int32, device=dev)

    CAND_CAP = 4096

    def new_candidate_set(self):
        """Per-batch candidate lists the scoring kernel fills (dlpd_zifft_filter_cand) and select() consumes."""
        return {"keys": torch.empty(self.batch * self.CAND_CAP, dtype=torch.int64, device=self.device),
                "count": torch.zeros(2 * self.batch, dtype=torch.int32, device=self.device), "cap": self.CAND_CAP}

    def reset(self):
        self.lib.call("dlpd_topk_glist_reset", _ptr(self.glist), self.K, _stream(self.device))
        self.tau.zero_()

    # Overflowed candidate lists are rebuilt from the restraints' bounding cubes while those hold at most this many voxels
    # (one block per rotation walks them): 65^3, the largest cube at which a rebuilt launch was measured and found no slower
    # than the full path on the same rotations (EXPERIMENTS.md RESTRAINTS); above it, and with None, only thinning runs
    REBUILD_LIMIT = 65 ** 3

    def set_restraints(self, table):
        """table: a ``Utils.Restraints.RestraintTable`` for the whole rotation set (or None: no restraints, exactly the calls
        of a free search).  Uploaded once; settable between searches."""
        self.restraints = table
        self._rst = None
        if table is not None:
            self._rst = (torch.from_numpy(table.centres.copy()).to(self.device), torch.from_numpy(table.bounds.copy()).to(self.device))

    def select(self, V, nb, cset=None, rot_ids=None):
        """V (nb, nvox) contiguous -> (scores, flat indices) (nb, K) in the reference's pick order.
        cset: the candidate set the scoring kernel filled for exactly these nb rotations (or None).

        Contract WITH a cset (the steady-state path of ``DockingEngine.step``): a rotation whose candidate list is
        valid comes back with only the picks that can still enter the running list -- the scores <= tau (the K-th
        score published by the last merge), in pick order, the rest of its row padded with +inf / index 0 -- which is
        exactly what ``merge()`` needs and NOT the reference's full K picks (Docker.py:89-98); rotations without a valid
        list (list not yet full, tau >= 0, overflow) get the full radix select.  A cset is SINGLE-USE: the select
        consumes and resets its counters, so it must be refilled by the scoring kernel before the next select.  Callers
        that want the reference's K picks per rotation pass ``cset=None``.

        With ``exclusion`` r > 0 the picks are those of suppress_r(V) (include/dlpd.h): V is a batch of cubes, its
        local-minimum copy Vs is what the radix select reads, and the complete candidate lists are thinned in place.

        With restraints set (``set_restraints``) the picks are those of restrain(V): ``rot_ids`` -- the batch's global rotation
        indices, int32 on the device, what ``merge`` gets -- index the table; the complete candidate lists lose what is not
        allowed, the overflowed ones are rebuilt from the allowed region, and Vs is masked for the rest.  Both: the
        intersection, a local minimum of the unrestricted V that is allowed."""
        nvox = V[0].numel()
        r = int(self.exclusion)
        tab = self.restraints
        if r < 0:
            raise RuntimeError("dlpd: exclusion radius %r (0 = none, the reference; 1..4 voxels)" % (self.exclusion,))
        if r > 0 or tab is not None:
            n = int(round(nvox ** (1.0 / 3.0)))
            if n * n * n != nvox:
                raise RuntimeError("dlpd: %s needs cubic score volumes, got %d voxels per rotation" %
                                   ("an exclusion radius" if r > 0 else "a restraint set", nvox))
            if tab is not None and rot_ids is None:
                raise RuntimeError("dlpd: a restrained select needs rot_ids, the batch's global rotation indices")
            if tab is not None and n % 2:
                raise RuntimeError("dlpd: a restraint set needs score volumes of even side, got %d" % n)
            if self._Vs is None or self._Vs.shape[1] != nvox:
                self._Vs = torch.empty(self.batch, nvox, dtype=torch.float32, device=self.device)
            st = _stream(self.device)
            cc, cap = (_ptr(cset["count"]), cset["cap"]) if cset is not None else (0, 0)
            src = V
            if tab is not None:
                rst = (_ptr(rot_ids), _ptr(self._rst[0]), _ptr(self._rst[1]), tab.J, tab.need)
                if cset is not None:
                    rebuild = self.REBUILD_LIMIT is not None and tab.cube_volume() <= self.REBUILD_LIMIT
                    self.lib.call("dlpd_topk_restrain_cand", _ptr(V), nb, n, *rst, _ptr(self.tau) if rebuild else 0,
                                  _ptr(cset["keys"]), cc, cap, st)
            if r > 0:
                self.lib.call("dlpd_topk_suppress", _ptr(V), _ptr(self._Vs), nb, n, r, cc, cap, st)
                if cset is not None:
                    self.lib.call("dlpd_topk_suppress_cand", _ptr(V), nb, n, r, _ptr(cset["keys"]), cc, cap, st)
                src = self._Vs
            if tab is not None:
                self.lib.call("dlpd_topk_restrain", _ptr(src), _ptr(self._Vs), nb, n, *rst, cc, cap, st)
            V = self._Vs
        if cset is None:
            self.lib.call("dlpd_topk_select", _ptr(V), nb, nvox, self.K, _ptr(self.cand_score), _ptr(self.cand_idx),
                          _ptr(self.ws), _stream(self.device))
        else:
            self.lib.call("dlpd_topk_select_cand", _ptr(V), nb, nvox, self.K, _ptr(self.cand_score), _ptr(self.cand_idx),
                          _ptr(self.ws), _ptr(cset["keys"]), _ptr(cset["count"]), cset["cap"], _stream(self.device))
        return self.cand_score[:nb], self.cand_idx[:nb]

    def merge(self, rot_ids, nb):
        """rot_ids int32 (nb,) on the device, ascending."""
        self.lib.call("dlpd_topk_merge_tau", _ptr(self.cand_score), _ptr(self.cand_idx), _ptr(rot_ids), nb, self.K,
                      _ptr(self.glist), _ptr(self.tau), _stream(self.device))

    def entries(self, glist=None):
        """-> (rot, flat_idx, score, pick) numpy arrays sorted as the reference's top_list."""
        g = (self.glist if glist is None else glist).cpu().numpy().view(np.uint64)
        count = int(g[0])
        hi = g[2:2 + count]
        lo = g[2 + self.K:2 + self.K + count]
        score = key_to_float((hi >> np.uint64(32)).astype(np.uint32)).copy()
        negzero = ((lo >> np.uint64(31)) & np.uint64(1)).astype(bool)
        score[negzero] = np.float32(-0.0)
        rot = (hi & np.uint64(0xFFFFFFFF)).astype(np.int64)
        idx = (lo & np.uint64(0x7FFFFFFF)).astype(np.int64)
        pick = (lo >> np.uint64(32)).astype(np.int64)
        return rot, idx, score, pick

    @staticmethod
    def merge_entries(parts, K):
        """Deterministic merge of several ranks' lists: sort by (score, rotation, pick), keep K.
        Exact because the global top-K is a subset of the union of per-shard top-Ks and the key
        reproduces the reference's stable insertion order."""
        rot = np.concatenate([p[0] for p in parts])
        idx = np.concatenate([p[1] for p in parts])
        score = np.concatenate([p[2] for p in parts])
        pick = np.concatenate([p[3] for p in parts])
        order = np.lexsort((pick, rot, score + np.float32(0.0)))[:K]
        return rot[order], idx[order], score[order], pick[order]

    @staticmethod
    def to_top_list(entries, N):
        rot, idx, score, _ = entries
        x, y, z = idx // (N * N), (idx // N) % N, idx % N
        return [(int(rot[i]), int(x[i]), int(y[i]), int(z[i]), float(score[i])) for i in range(len(rot))]


class _Grid:
    """What one resolution grid of a search owns: the fine grid, or the coarse grid of the two-resolution model (half the
    box, score channels only).  Sizes, pivot, crop and rotation scale; the ligand (and its channels-last or quad copy K1
    gathers from), the receptor spectrum K2 reads, the K1 -> K2 workspaces; the state of the sparse K1 (set_ligand)."""

    def __init__(self, eng, L, C, CT, center, extent, rot_scale, packed_receptor):
        lib, dev, nb, f32 = eng.lib, eng.device, eng.batch, torch.float32
        self.L, self.N, self.NZ, self.C, self.CT = L, 2 * L, L + 1, C, CT
        self.center = float(L) / 2.0 if center is None else float(center)
        self.extent, self.rot_scale = extent, float(rot_scale)
        N, NZ = self.N, self.NZ
        self.lig = torch.zeros(CT, L, L, L, dtype=f32, device=dev)
        # ... in chunk-major order where the engine asks for it or the library prefers it at this box (include/dlpd.h,
        # dlpd_make_channel_chunks); the role-split K1 formulation reads the channels-last order only
        want = eng.k1_chunk_major if eng.k1_chunk_major is not None else bool(lib.call("dlpd_channel_chunks_default", L))
        self.chunk_major = bool(eng.use_cl and want and eng._k1_form_at(L) in (0, 1))
        self.ligcl = torch.empty(lib.call("dlpd_channel_chunks_floats" if self.chunk_major else "dlpd_channels_last_floats", C, L),
                                 dtype=f32, device=dev) if eng.use_cl else None
        self.ligq = torch.empty(lib.call("dlpd_quads_floats", CT, L), dtype=f32, device=dev) if eng.use_quads else None
        # boxes whose K2 re-reads the receptor spectrum for every rotation (80, 40) take a copy in the order its column
        # phase consumes it (include/dlpd.h: dlpd_receptor_pack); written by set_receptor, read by untransposed launches
        npk = lib.call("dlpd_receptor_packed_floats", CT, L) if packed_receptor else 0
        self.recP = torch.zeros(npk, dtype=f32, device=dev) if npk else None
        self.recF = None if (eng._spectrum_is_temporary and self.recP is not None) else \
            torch.zeros(CT, NZ, N, N, 2, dtype=f32, device=dev)
        # boxes 64 / 32 (K2 keeps a rotation's receptor values in registers): a copy in the order of K2's receptor fetches
        # (include/dlpd.h: dlpd_receptor_order), read by untransposed launches; the natural spectrum stays for the others
        nord = lib.call("dlpd_receptor_ordered_floats", CT, L) if packed_receptor else 0
        self.recO = torch.zeros(nord, dtype=f32, device=dev) if nord else None
        self.wsA = torch.empty(nb * CT * NZ * L * L * 2, dtype=f32, device=dev)
        self.wsB = torch.empty(nb * CT * NZ * N * N * 2, dtype=f32, device=dev)
        # sparse K1: the ligand's cell map, the per-rotation maps, their pencil words (K2 goes by them where it reads
        # the packed receptor), the decision and the fraction of cells occupied -- set by set_ligand
        self.pencil_map_ok = self.recP is not None and bool(lib.call("dlpd_pencil_map_supported", L))
        self.occ_src = self.occ_rot = self.pen = self.fill = None
        self.sparse = self.pencil_map = False


class DockingEngine:
    """Exhaustive translation scoring for batches of rotations of ONE receptor/ligand pair.

    Parameters follow the reference objects: ``W1,b1,W2,b2`` are SimpleFilter.fc[0]/fc[2]
    (DockingModels.py:28-32), ``clip`` the VolumeConvolution(clip) of DockingModels.py:48,
    ``threshold_clash`` Docker.py:226, ``max_conf`` Docker.py:26.
    """

    def __init__(self, L, C, W1, b1, W2, b2, clip=5.0, threshold_clash=300.0, has_clash=True,
                 max_conf=1000, batch=8, device="cuda", lib=None, center=None, coarse_channels=0,
                 fine_unfused=None, channels_last=None, k3_form=0, coarse_center=None, extent=None,
                 orient=True, quads=True, prefilter=True, packed_receptor=True,
                 rotation_scale=1.0, coarse_rotation_scale=None, rotation_axis_order="xyz", clip_mode="output",
                 rotation_transpose=False, keep_receptor_spectrum=False, k1_form=0, sparse_k1=None,
                 k1_chunk_major=None, exclusion=0, restraints=None):
        """coarse_channels > 0: the reference's two-resolution layout -- C channels at L^3 plus
        ``coarse_channels`` at (L/2)^3 (ProteinRepresentationModels.py:72-76); W1 is (H, C+coarse).
        extent < L: the volumes are extent^3 boxes in the corner of the L^3 ones (a box size without a compiled plan
        inside this one, Docker._search_plan): rotated ligand volumes are cropped to that box (coarse grid:
        extent / 2), ``center`` / ``coarse_center`` are the pivots of the small boxes."""
        self.device = torch.device(device)
        if lib is None:
            if self.device.type != "cuda":
                raise RuntimeError("dlpd: the product path runs on an AMD GPU only "
                                   "(no CPU fallback); got device %s" % self.device)
            lib = get_lib()
        self.lib = lib
        if not lib.call("dlpd_grid_supported", int(L)):
            raise RuntimeError("dlpd: box size L=%d has no compiled fused pipeline" % L)
        self.L, self.N, self.C = int(L), 2 * int(L), int(C)
        self.has_clash = bool(has_clash)
        self.CT = self.C + (1 if self.has_clash else 0)
        # Conventions of the volume rotation and of VolumeConvolution(clip) that TorchProteinLibrary may define
        # differently (Utils/Conventions.py): scale + axis order are folded into the 3x3 maps K1 samples with.  The clash
        # channel follows where it comes from: re-projected ATOMS (clash_provider, the reference's own path,
        # Docker.py:221-224) are rotated geometrically by the TRUE R; a stored forbidden VOLUME (dock_volumes without a
        # provider -- the synthetic configs) is a volume like the others and turns with the mapped matrix; clip_mode "input" clamps the receptor once
        # and every rotated ligand batch before its transform (through the volumes path: exact, one extra round trip of
        # the rotated volumes -- the price of a convention nobody has confirmed), "none" drops the clamp.
        rot_scale1 = float(rotation_scale if coarse_rotation_scale is None else coarse_rotation_scale)
        self.rot_axis_order, self.rot_transpose = rotation_axis_order, bool(rotation_transpose)
        self._rot_mapped = float(rotation_scale) != 1.0 or rot_scale1 != 1.0 or rotation_axis_order != "xyz" or self.rot_transpose
        if clip_mode not in ("output", "input", "none"):
            raise RuntimeError("dlpd: clip_mode %r" % (clip_mode,))
        self.clip_mode = clip_mode
        self.clip = clip
        self.threshold = float(threshold_clash)
        self.K = int(max_conf)
        self.batch = int(batch)
        # exclusion radius of the search in voxels (include/dlpd.h, dlpd_topk_suppress; build-defined, 0 = the reference's
        # list): read at reset_top(), so a live engine serves searches with different radii
        self.exclusion = int(exclusion)
        # distance restraints of the search (Utils.Restraints.RestraintTable over the whole rotation set, or None; build-defined):
        # read at reset_top(), as the radius is
        self.restraints = restraints
        dev = self.device
        f32 = torch.float32
        self.C1 = int(coarse_channels)
        # kernel formulation of the fused K3 (include/dlpd.h, dlpd_zifft_filter_form): 0 = the library's default
        # (role-split transform / filter waves where compiled), 1 = channel-owning waves; same results bit for bit
        self.k3_form = int(k3_form)
        # kernel formulation of the channels-last K1 (include/dlpd.h, dlpd_zfft_channels_last_form): 0 = the library's
        # default, 1 = every wave gathers / transforms / stores in turn, 2 = role-split (boxes 64 and 80); same bits
        self.k1_form = int(k1_form)
        if self.k1_form not in (0, 1, 2):
            raise RuntimeError("dlpd: k1_form %r (0 = library default, 1 = phased, 2 = role-split)" % (k1_form,))
        if self.k1_form == 2 and int(L) in (64, 80) and not lib.call("dlpd_k1_form_supported", int(L), 2):
            # form 2 is a TEST-VARIANT kernel (-DDLPD_TEST_VARIANTS builds: tests/variants/libdlpd_variants.so): the product
            # library refuses it at the first launch -- say so when the engine is built, not in the middle of a search
            raise RuntimeError("dlpd: k1_form=2 (role-split K1) exists in -DDLPD_TEST_VARIANTS builds only; this library "
                               "(%s) does not hold it" % getattr(lib, "path", "?"))
        # fine_unfused (diagnostic / A-B): materialise the real correlations of the fine grid and run the
        # vectorised filter kernel behind a plain z-inverse, instead of the fused z-inverse + MLP (K3)
        self.fine_unfused = bool(fine_unfused)
        self.set_filter(W1, b1, W2, b2)
        nb, CT, N = self.batch, self.CT, self.N
        self.V = torch.empty(nb, N, N, N, dtype=f32, device=dev)
        # channels-last gather (include/dlpd.h): one 16-byte load serves four channels of a corner, so the rotation
        # costs the same for every rotation; slab orientation and the quad layout are the per-channel kernel's
        # remedies and stay for ligands with few channels (and as diagnostic switches)
        # Kernel choices are CONSTRUCTOR ARGUMENTS only (no switch is read from outside the call): channels_last (default: ligands with
        # >= 8 channels), orient / quads (the per-channel K1's launch variants), prefilter (top-K candidate lists from
        # K3).  They select equivalent kernels, never less work; ``switches()`` reports what is active.
        if channels_last is None:
            channels_last = self.C >= 8
        self.use_cl = bool(channels_last)
        # source layout of the channels-last K1: None = the library's choice per box, True / False = the chunk-major copy
        # ([chunk][x][y][z][CC]) or the channels-last one ([x][y][z][Cp]) on every grid; same spectra either way
        self.k1_chunk_major = None if k1_chunk_major is None else bool(k1_chunk_major)
        self.extent = int(extent) if extent and int(extent) < int(L) else 0
        if self.extent and self.clip_mode == "input":
            raise RuntimeError("dlpd: clip_mode 'input' is not combined with embedded boxes (use a compiled box size)")
        # (slab orientation needs K2's transposed reader: every compiled box except 80 in libdlpd.so)
        self.orient = bool(orient) and not self.use_cl and bool(lib.call("dlpd_orientation_supported", int(L)))
        self.use_quads = bool(quads) and not self.use_cl and not self.extent
        # With the channels-last K1 every launch is untransposed and goes through the staged path, so where K2 reads the
        # PACKED receptor copy (boxes 80 / 40) the natural-layout spectrum is dead once it has been packed: it becomes a
        # temporary of set_receptor instead of a second resident copy (282 MB at 17 channels, 813 MB at 49, box 80).
        self._spectrum_is_temporary = bool(self.use_cl and not keep_receptor_spectrum)
        self.prefilter = bool(prefilter)
        # Search-side sparsity (round 6): a ligand whose channels are zero in most 4^3 cells of its box (any real protein's
        # representation) gets per-rotation occupancy maps, and the channels-last K1 skips what they mark empty -- same
        # spectra.  None: decided per ligand and grid in set_ligand (on where the ligand's cells, dilated by one, stay below
        # SPARSE_K1_MAX_FILL of the box); True / False force it.
        self.sparse_k1_wanted = sparse_k1
        self.window = None
        if self.extent:
            # the reference's (2 extent)^3 translation grid inside this engine's (2L)^3 one: index t for 0 <= t <= extent
            # (t = extent: no overlap), 2L + t for -extent < t < 0 -- monotonic, so equal scores keep the reference's order.
            # The top-K takes the gathered grid; K3's candidate lists carry indices of the large grid and are not used.
            e = self.extent
            self.window = torch.tensor(list(range(0, e + 1)) + list(range(2 * int(L) - (e - 1), 2 * int(L))), dtype=torch.long, device=dev)
            # ... as ONE flat gather index over the (2L)^3 volume (the three per-axis index_selects it replaces made
            # three passes over the score volume per batch)
            w, Nn = self.window, 2 * int(L)
            self.window_flat = ((w[:, None, None] * Nn + w[None, :, None]) * Nn + w[None, None, :]).reshape(-1).contiguous()
            self.prefilter = False
        self.fine = _Grid(self, self.L, self.C, CT, center, self.extent, rotation_scale, packed_receptor)
        self.coarse = None
        if self.C1:
            L1 = self.L // 2
            if self.L % 2 or not lib.call("dlpd_grid_supported", L1):
                raise RuntimeError("dlpd: coarse box size %d has no compiled pipeline" % L1)
            self.coarse = _Grid(self, L1, self.C1, self.C1, coarse_center, self.extent // 2, rot_scale1, packed_receptor)
            # first-layer pre-activations of the coarse channels on the coarse grid (dlpd_zifft_preact): HP planes
            self.pre = torch.empty(nb, self.HP, 2 * L1, 2 * L1, 2 * L1, dtype=f32, device=dev)
        self.grids = [g for g in (self.fine, self.coarse) if g is not None]
        if self.fine_unfused:
            self.conv = torch.empty(nb, CT, N, N, N, dtype=f32, device=dev)
        self.top = DeviceTopList(self.K, nb, dev, lib)
        # optional: callable(R (nb,3,3) f32 device) -> (nb,L,L,L) f32 device ligand forbidden volumes
        # re-projected from rotated ATOMS (Docker.py:221-224) instead of the rotated volume
        self.clash_provider = None
        # step()'s double buffer, made at the first step (_start_steps); the batch whose select + merge is not issued yet
        self._Vbuf = self._side = self._pending = None

    @property
    def _out_clip(self):
        """(has_clip, clip) of the kernels' clamp on the correlation OUTPUT."""
        on = self.clip is not None and self.clip_mode == "output"
        return (1 if on else 0), float(self.clip if on else 0.0)

    @property
    def _in_clip(self):
        return float(self.clip) if (self.clip is not None and self.clip_mode == "input") else None

    def _kernel_R(self, R, g):
        """The 3x3 maps K1 samples with on grid g: R itself, or scale * P R P (Utils/Conventions.kernel_matrices)."""
        if not self._rot_mapped:
            return R
        from .Utils.Conventions import kernel_matrices
        return kernel_matrices(R, g.rot_scale, self.rot_axis_order, self.rot_transpose)

    def _k1_form_at(self, L):
        """The requested K1 formulation where the library holds both (boxes 64, 80); its only one elsewhere."""
        return self.k1_form if int(L) in (64, 80) else 0

    def switches(self):
        """Which of the equivalent kernel formulations and which conventions this engine launches with (bench.py records it)."""
        fine, c = self.fine, self.coarse
        layout = lambda g: None if not (g and self.use_cl) else ("chunk_major" if g.chunk_major else "channels_last")
        return {"k1": "channels_last" if self.use_cl else "per_channel",
                "k1_source_layout": {"fine": layout(fine), "coarse": layout(c)},
                "k1_slab_orientation": bool(self.orient), "k1_quad_layout": bool(self.use_quads),
                "k1_form": {0: "library default", 1: "phased", 2: "role-split"}[self.k1_form],
                "k3_form": {0: "library default (role-split where compiled)", 1: "channel-owning", 2: "role-split"}[self.k3_form],
                "k3_unfused": bool(self.fine_unfused), "topk_candidate_lists": bool(self.prefilter),
                "exclusion": int(self.exclusion),
                "restraints": None if self.restraints is None else (self.restraints.J, self.restraints.need),
                "k2_packed_receptor": {"fine": fine.recP is not None, "coarse": bool(c and c.recP is not None)},
                "k2_ordered_receptor": {"fine": fine.recO is not None, "coarse": bool(c and c.recO is not None)},
                "embedded_extent": self.extent or None,
                "k1_occupancy_maps": {"fine": fine.sparse, "coarse": bool(c and c.sparse),
                                      "k2_pencil_map": {"fine": fine.pencil_map, "coarse": bool(c and c.pencil_map)},
                                      "ligand_cells_occupied": {"fine": fine.fill, "coarse": c.fill if c else None}},
                "rotation": {"center": fine.center, "scale": fine.rot_scale, "axis_order": self.rot_axis_order,
                             "transpose": self.rot_transpose},
                "clip_mode": self.clip_mode}

    # ---- inputs ------------------------------------------------------------------------
    def set_filter(self, W1, b1, W2, b2):
        """SimpleFilter parameters (DockingModels.py:28-32) in the kernels' layout: W1 transposed and zero-padded to
        the hidden width the filter kernel is compiled for.  May be called again on a live engine (same shapes)."""
        f32, dev, lib = torch.float32, self.device, self.lib
        W1 = torch.as_tensor(W1, dtype=f32).reshape(-1, self.C + self.C1)
        H = W1.shape[0]
        HP = lib.call("dlpd_fused_hidden_pad", int(H), self.L, int(self.C1 > 0))
        if HP < 0:
            raise RuntimeError("dlpd: hidden width %d has no fused filter kernel at box %d" % (H, self.L))
        if HP > 32 and (self.fine_unfused or self.k3_form == 1):
            raise RuntimeError("dlpd: hidden width %d runs on the role-split K3 only" % H)
        if getattr(self, "HP", HP) != HP:
            raise RuntimeError("dlpd: a live engine keeps its hidden width (%d), got %d" % (self.HP, HP))
        self.H, self.HP = H, HP
        W1t = torch.zeros(self.C + self.C1, HP, dtype=f32)
        W1t[:, :H] = W1.t()
        b1p = torch.zeros(HP, dtype=f32)
        b1p[:H] = torch.as_tensor(b1, dtype=f32).reshape(-1)
        W2p = torch.zeros(HP, dtype=f32)
        W2p[:H] = torch.as_tensor(W2, dtype=f32).reshape(-1)
        self.W1t, self.b1, self.W2 = W1t.to(dev), b1p.to(dev), W2p.to(dev)
        self.b2 = float(torch.as_tensor(b2).reshape(-1)[0])

    def set_receptor(self, rec_volumes, rec_forbidden=None, rec_coarse=None):
        """rec_volumes (C,L,L,L); rec_forbidden (L,L,L); rec_coarse (C1,L/2,..).  Spectra precomputed
        once per pair (the reference recomputes them every batch inside VolumeConvolution,
        DockingModels.py:71)."""
        f32, dev, clip = torch.float32, self.device, self._in_clip
        clamp = (lambda t: t) if clip is None else (lambda t: t.clamp(-clip, clip))
        L, C = self.L, self.C
        rec = torch.zeros(self.CT, L, L, L, dtype=f32, device=dev)
        rec[:C] = clamp(torch.as_tensor(rec_volumes, dtype=f32).reshape(C, L, L, L).to(dev))
        if self.has_clash:
            rec[C] = torch.as_tensor(rec_forbidden, dtype=f32).reshape(L, L, L).to(dev)
        inputs = [(self.fine, rec)]
        if self.coarse:
            L1 = self.coarse.L
            inputs.insert(0, (self.coarse, clamp(torch.as_tensor(rec_coarse, dtype=f32).reshape(self.C1, L1, L1, L1).to(dev)).contiguous()))
        st = _stream(dev)
        for g, r in inputs:
            recF = g.recF if g.recF is not None else torch.empty(g.CT, g.NZ, g.N, g.N, 2, dtype=f32, device=dev)
            self.lib.call("dlpd_rfft3d_padded", _ptr(r), _ptr(recF), _ptr(g.wsA), g.CT, g.L, 1.0 / float(g.N) ** 3, st)
            if g.recP is not None:
                self.lib.call("dlpd_receptor_pack", _ptr(recF), _ptr(g.recP), g.CT, g.L, st)
            if g.recO is not None:
                self.lib.call("dlpd_receptor_order", _ptr(recF), _ptr(g.recO), g.CT, g.L, st)

    SPARSE_K1_MAX_FILL = 0.7

    def _ligand_occupancy(self):
        """Cell maps of the stored ligand (all score channels) and the decision whether K1 goes by per-rotation maps."""
        from . import ops
        for g in self.grids:
            g.sparse = g.pencil_map = False
        if not self.use_cl or self.sparse_k1_wanted is False:
            return

        def reach(occ):
            """Fraction of the cells a ROTATED copy can mark: the per-rotation maps are conservative by about one cell per
            side, so the decision goes by the ligand's cells dilated by one (a 60 %-full coarse grid marks everything)."""
            o = occ.to(torch.float32).reshape(1, 1, *occ.shape[-3:])
            return float(torch.nn.functional.max_pool3d(o, kernel_size=3, stride=1, padding=1).mean())
        for g in self.grids:
            g.occ_src = ops.tile_occupancy(g.lig[: g.C].unsqueeze(0), lib=self.lib)
            g.fill = float(g.occ_src.float().mean())
            g.sparse = bool(self.sparse_k1_wanted) or reach(g.occ_src) < self.SPARSE_K1_MAX_FILL
            if g.sparse and g.occ_rot is None:
                nc = (g.L + 3) // 4
                g.occ_rot = torch.empty(self.batch, nc, nc, nc, dtype=torch.uint8, device=self.device)
                g.pen = torch.empty(self.batch, nc, dtype=torch.int32, device=self.device)
            # Where K2 reads the packed receptor (boxes 80 / 40) it can go by a per-rotation PENCIL map: K1 then does not
            # write the blocks without an occupied cell and K2 does not read the pencils the map marks empty (same spectra,
            # same lists)
            g.pencil_map = g.sparse and g.pencil_map_ok

    def set_ligand(self, lig_volumes, lig_forbidden=None, lig_coarse=None):
        L, fine, coarse = self.L, self.fine, self.coarse
        if coarse:
            coarse.lig.copy_(torch.as_tensor(lig_coarse, dtype=torch.float32).reshape(coarse.lig.shape))
        fine.lig[: self.C] = torch.as_tensor(lig_volumes, dtype=torch.float32).reshape(self.C, L, L, L).to(self.device)
        if self.has_clash:
            fine.lig[self.C] = torch.as_tensor(lig_forbidden, dtype=torch.float32).reshape(L, L, L).to(self.device)
        # the layout the rotation gather reads (include/dlpd.h), once per pair: channels-last, or quads (4x the ligand's bytes)
        st = _stream(self.device)
        for g in self.grids:
            if self.use_cl:
                self.lib.call("dlpd_make_channel_chunks" if g.chunk_major else "dlpd_make_channels_last", _ptr(g.lig), _ptr(g.ligcl),
                              g.C, g.L, st)
            elif self.use_quads:
                self.lib.call("dlpd_make_quads", _ptr(g.lig), _ptr(g.ligq), g.CT, g.L, st)
        self._ligand_occupancy()

    @staticmethod
    def prefers_quads(R):
        """(n,3,3) -> bool (n,): after the slab orientation the source z axis is carried by the in-plane
        x/y axis rather than by the output z axis.  For those rotations the quad-layout gather
        (include/dlpd.h) is ~1.4x faster; for the others the plain volume (4x fewer bytes, L2 resident)
        is as good or better inside the full pipeline."""
        R = np.asarray(R)
        inplane = np.maximum(np.abs(R[:, 0, 2]), np.abs(R[:, 1, 2]))
        return inplane > np.abs(R[:, 2, 2])

    @staticmethod
    def prefers_transposed(R):
        """(n,3,3) rotation matrices -> bool (n,): the source z axis is closer to the output x axis than to
        the output y axis, i.e. the x-plane gather of K1 would run across memory rows (include/dlpd.h)."""
        R = np.asarray(R)
        return np.abs(R[:, 0, 2]) > np.abs(R[:, 1, 2])

    # ---- hot loop ------------------------------------------------------------------------
    def _k1(self, g, R, nb, tr, quads, nch, st):
        """K1 of grid g: rotation + z transform of its first nch ligand channels into channels [0, nch) of g.wsA, from the
        channels-last copy (by occupancy maps where the ligand is sparse; score channels only), the quad layout or the
        volume itself.  -> the pencil words K2 must go by (K1 left the pencils of empty blocks unwritten), or None."""
        call, L, c0 = self.lib.call, g.L, g.center
        if self.use_cl:
            if g.sparse and self._k1_form_at(L) in (0, 1):
                pen = g.pen if g.pencil_map else None
                call("dlpd_rotated_occupancy", _ptr(g.occ_src), _ptr(R), _ptr(g.occ_rot), _ptr(pen), nb, L, c0, st)
                call("dlpd_zfft_channel_chunks" if g.chunk_major else "dlpd_zfft_channels_last_occ", _ptr(g.ligcl), _ptr(R),
                     _ptr(g.occ_rot), _ptr(g.wsA), nb, g.C, g.CT, 0, L, c0, g.extent, int(g.pencil_map), st)
                return pen
            if g.chunk_major:
                call("dlpd_zfft_channel_chunks", _ptr(g.ligcl), _ptr(R), 0, _ptr(g.wsA), nb, g.C, g.CT, 0, L, c0, g.extent, 0, st)
                return None
            call("dlpd_zfft_channels_last_form", _ptr(g.ligcl), _ptr(R), _ptr(g.wsA), nb, g.C, g.CT, 0, L, c0, g.extent,
                 self._k1_form_at(L), st)
        elif quads:
            call("dlpd_zfft_quads", _ptr(g.ligq), _ptr(R), _ptr(g.wsA), nb, nch, g.CT, 0, L, c0, tr, st)
        else:
            call("dlpd_zfft_oriented_ext", _ptr(g.lig), _ptr(R), _ptr(g.wsA), nb, nch, g.CT, 0, L, 0, 1, c0, tr, g.extent, st)
        return None

    def _k1_volumes(self, g, vols, occ, st):
        """K1 of grid g for given volumes (nb, C, L, L, L): z transform of the score channels, by their occupancy maps
        if given.  -> the pencil words K2 must go by (where K2 reads the packed receptor, empty x-planes are not written
        and K2 goes by the maps' OR over z), or None."""
        call, nb, L = self.lib.call, vols.shape[0], g.L
        if occ is None:
            call("dlpd_zfft_into", _ptr(vols), 0, _ptr(g.wsA), nb, g.C, g.CT, 0, L, g.C * L ** 3, 0, 0.0, st)
            return None
        pen = None
        if g.pencil_map_ok:
            pen = torch.empty(nb, (L + 3) // 4, dtype=torch.int32, device=self.device)
            call("dlpd_pencil_bits", _ptr(occ), _ptr(pen), nb, L, st)
        call("dlpd_zfft_volumes_occ", _ptr(vols), _ptr(occ), _ptr(g.wsA), nb, g.C, g.CT, 0, L, g.C * L ** 3, int(pen is not None), st)
        return pen

    def _k2(self, g, nb, tr, pen, st):
        """Stage K2 of grid g on what K1 left in its wsA; tr: the slab orientation K1 used; pen: the pencil words K1
        returned (K2 takes the pencils they mark empty as zeros, score channels only)."""
        if pen is not None:
            assert g.recP is not None and not tr
            self.lib.call("dlpd_xy_correlate_packed_occ", _ptr(g.wsA), _ptr(g.recP), _ptr(g.wsB), nb, g.CT, g.L, _ptr(pen), g.C, st)
        elif g.recP is not None and not tr:
            self.lib.call("dlpd_xy_correlate_packed", _ptr(g.wsA), _ptr(g.recP), _ptr(g.wsB), nb, g.CT, g.L, st)
        elif g.recO is not None and not tr:
            self.lib.call("dlpd_xy_correlate_ordered", _ptr(g.wsA), _ptr(g.recO), _ptr(g.wsB), nb, g.CT, g.L, st)
        else:
            if g.recF is None:       # (packed-receptor boxes drop the natural-layout spectrum: keep_receptor_spectrum=True keeps it)
                raise RuntimeError("dlpd: this engine holds only the packed receptor spectrum; a transposed launch needs "
                                   "keep_receptor_spectrum=True")
            self.lib.call("dlpd_xy_correlate_oriented", _ptr(g.wsA), _ptr(g.recF), _ptr(g.wsB), nb, g.CT, g.L, 0, tr, st)

    def score_batch(self, R, mark=None, out=None, volumes=None, transposed=False, quads=False, cset=None, occupancy=None):
        """R (nb,3,3) float32 on the device, nb <= batch.  Returns V[:nb] (view of the engine's
        buffer, overwritten by the next call): Docker.py:218-232.  mark(name): optional callback
        after each stage (timing).
        volumes = (lig (nb,C,L,L,L), forbidden (nb,L,L,L) | None, coarse (nb,C1,L/2,..) | None): the
        batch's ligand volumes are given as they are (dockE3: re-projected and re-represented per
        rotation, Docker.py:163-172) instead of rotating the stored ligand by R.
        occupancy = (fine map, coarse map | None) with ``volumes``: uint8 (nb, ceil(L/4)^3) maps of the cells that hold a
        non-zero value (ops.conv3d(return_occupancy=True)); cells marked empty are never read -- the volumes may be
        unwritten there (ops.conv3d(unwritten=True)).
        transposed: slab orientation for ALL rotations of the batch (include/dlpd.h); search() groups the
        rotations for which it pays (prefers_transposed) into batches of their own."""
        self._cset_used = None
        if volumes is not None:
            return self._score_volumes(volumes, mark, out, cset, occupancy)
        nb = R.shape[0]
        assert nb <= self.batch and R.dtype == torch.float32 and R.is_contiguous()
        provider = self.clash_provider if self.has_clash else None
        if self._in_clip is not None:
            return self._score_rotated_then_clamped(R, mark, out, cset, provider)
        tr = int(bool(transposed) and self.orient)
        use_quads = bool(quads) and self.use_quads
        V = self.V if out is None else out
        call, st, L = self.lib.call, _stream(self.device), self.L
        fine, coarse = self.fine, self.coarse
        Rk, Rk1 = self._kernel_R(R, fine), (self._kernel_R(R, coarse) if coarse else None)
        self._keepR = (Rk, Rk1)                        # mapped copies stay alive until the stream has consumed them
        mark = mark or (lambda name: None)
        mark("begin")
        if coarse:
            # coarse resolution first: rotate + correlate + clip -> real volumes the fine filter reads
            pen = self._k1(coarse, Rk1, nb, tr, use_quads, coarse.C, st)
            sub = getattr(mark, "sub_stages", False)     # (diagnostic callers: a mark after every kernel of the coarse stage)
            if sub:
                mark("coarse_k1")
            self._k2(coarse, nb, tr, pen, st)
            if sub:
                mark("coarse_k2")
            self._coarse_preact(nb, st)
            mark("coarse")
        # the clash channel goes in the score channels' launch where it is the stored forbidden volume and K1 per-channel;
        # from re-projected rotated ATOMS (Docker.py:221-224) or beside the channels-last K1 it takes a launch of its own
        forb = provider(R).reshape(nb, L, L, L).contiguous() if provider is not None else None
        clash_apart = forb is not None or self.use_cl
        pen = self._k1(fine, Rk, nb, tr, use_quads, fine.C if clash_apart else fine.CT, st)
        if forb is not None:                  # same orientation as the score channels
            call("dlpd_zfft_oriented", _ptr(forb), 0, _ptr(fine.wsA), nb, 1, fine.CT, fine.C, L, L ** 3, 0, 0.0, tr, st)
        elif clash_apart and self.has_clash:  # the ligand's forbidden volume: one channel, per-channel kernel
            call("dlpd_zfft_oriented_ext", fine.lig.data_ptr() + self.C * L ** 3 * 4, _ptr(Rk), _ptr(fine.wsA), nb, 1,
                 fine.CT, fine.C, L, 0, 1, fine.center, 0, fine.extent, st)
        mark("k1_rotate_zfft")
        return self._correlate_and_filter(nb, V, mark, tr, cset, pen)

    def _score_volumes(self, volumes, mark, out, cset=None, occupancy=None):
        vl, vf, vc = volumes
        nb, L = vl.shape[0], self.L
        assert nb <= self.batch
        fine, coarse = self.fine, self.coarse
        occ0, occ1 = occupancy if occupancy is not None else (None, None)
        if (occ0 is not None or occ1 is not None) and self._in_clip is not None:
            raise RuntimeError("dlpd: occupancy maps are not combined with clip_mode 'input' (the clamp reads every voxel)")

        def _occ(o, n, Lx):
            if o is None:
                return None
            nc = (Lx + 3) // 4
            if o.dtype != torch.uint8 or o.device.type != self.device.type or o.numel() != n * nc ** 3:
                raise RuntimeError("dlpd: occupancy map %s does not belong to %d volumes of box %d" % (tuple(o.shape), n, Lx))
            return o.contiguous()
        occ0, occ1 = _occ(occ0, nb, L), (_occ(occ1, nb, coarse.L) if coarse else None)
        f32c = lambda t: t.to(device=self.device, dtype=torch.float32).contiguous()
        call, st = self.lib.call, _stream(self.device)
        V = self.V if out is None else out
        mark = mark or (lambda name: None)
        mark("begin")
        if self._in_clip is not None:                  # VolumeConvolution(clip) clamping its INPUTS (clip_mode "input")
            vl = f32c(vl).clamp(-self._in_clip, self._in_clip)
            vc = f32c(vc).clamp(-self._in_clip, self._in_clip) if coarse else vc
        pen1 = None
        if coarse:
            L1 = coarse.L
            vc = f32c(vc).reshape(nb, self.C1, L1, L1, L1)
            pen1 = self._k1_volumes(coarse, vc, occ1, st)
            self._k2(coarse, nb, 0, pen1, st)
            self._coarse_preact(nb, st)
            mark("coarse")
        vl = f32c(vl).reshape(nb, self.C, L, L, L)
        pen = self._k1_volumes(fine, vl, occ0, st)
        if self.has_clash:
            vf = f32c(vf).reshape(nb, L, L, L)
            call("dlpd_zfft_into", _ptr(vf), 0, _ptr(fine.wsA), nb, 1, fine.CT, fine.C, L, L ** 3, 0, 0.0, st)
        mark("k1_rotate_zfft")
        self._keep = (vl, vf, vc, occ0, occ1, pen, pen1)   # inputs and pencil words stay alive until the stream has consumed them
        return self._correlate_and_filter(nb, V, mark, 0, cset, pen)

    def _score_rotated_then_clamped(self, R, mark, out, cset, provider):
        """clip_mode "input": the reference order is rotate (Docker.py:218) -> VolumeConvolution(clip) (DockingModels.py:71),
        so the clamp acts on the ROTATED ligand volumes: they are materialised by the stand-alone rotation kernel, clamped
        (in _score_volumes) and fed to the pipeline as given volumes.  The clash channel is never clamped (Docker.py:32,225:
        VolumeConvolution() without clip)."""
        nb, st, fine, coarse = R.shape[0], _stream(self.device), self.fine, self.coarse
        Rk, Rk1 = self._kernel_R(R, fine), (self._kernel_R(R, coarse) if coarse else None)
        self._keepR = (Rk, Rk1)                        # alive until the stream has consumed them

        def rotated(g, Rg, c0, nch):
            v = torch.empty(nb, nch, g.L, g.L, g.L, dtype=torch.float32, device=self.device)
            self.lib.call("dlpd_rotate_trilinear", g.lig.data_ptr() + c0 * g.L ** 3 * 4, _ptr(Rg), _ptr(v), nb, nch, g.L, 0,
                          g.center, st)
            return v
        vl = rotated(fine, Rk, 0, self.C)
        vf = vc = None
        if self.has_clash:
            vf = provider(R).reshape(nb, self.L, self.L, self.L).contiguous() if provider is not None else rotated(fine, Rk, self.C, 1)
        if coarse:
            vc = rotated(coarse, Rk1, 0, self.C1)
        return self._score_volumes((vl, vf, vc), mark, out, cset)

    def _coarse_preact(self, nb, st):
        """Coarse grid, last stage: z-inverse + clip fused with the coarse half of the (linear) first layer
        (DockingModels.py:74-83): HP pre-activation planes on the coarse grid instead of C1 correlation volumes."""
        has_clip, clip = self._out_clip
        self.lib.call("dlpd_zifft_preact_form", _ptr(self.coarse.wsB), _ptr(self.pre), nb, self.C1, self.coarse.L,
                      self.W1t.data_ptr() + self.C * self.HP * 4, _ptr(self.b1), self.HP, has_clip, clip, self.k3_form, st)

    def _correlate_and_filter(self, nb, V, mark, tr, cset, pen):
        """K2 + K3 (+ filter) on whatever K1 left in the fine wsA (and the coarse result in aux); tr: the slab
        orientation K1 used; pen: the pencil words K1 returned."""
        has_clip, clip = self._out_clip
        call, st, L, fine = self.lib.call, _stream(self.device), self.L, self.fine
        self._k2(fine, nb, tr, pen, st)
        mark("k2_xy_corr")
        aux, C1, N1 = (_ptr(self.pre), self.C1, self.coarse.N) if self.coarse else (0, 0, 0)
        if self.fine_unfused:
            N3 = self.N ** 3
            call("dlpd_zifft_real_part", _ptr(fine.wsB), _ptr(self.conv), nb, self.CT, self.C, L, has_clip, clip, st)
            mark("k3_zifft")
            mask = self.conv.data_ptr() + self.C * N3 * 4 if self.has_clash else 0
            call("dlpd_filter_volumes", _ptr(self.conv), self.C, self.CT * N3, self.N, aux, C1, N1, int(C1 > 0), mask,
                 self.CT * N3, self.threshold, int(self.has_clash), _ptr(self.W1t), _ptr(self.b1), _ptr(self.W2),
                 self.b2, self.HP, _ptr(V), nb, st)
            mark("filter")
        else:
            # fused K3; with a candidate set it also appends every score below the running K-th one to the batch's
            # candidate lists, which the top-K select then takes instead of a radix select over V
            tau, ck, cc, cap = (_ptr(self.top.tau), _ptr(cset["keys"]), _ptr(cset["count"]), cset["cap"]) if cset else (0, 0, 0, 0)
            call("dlpd_zifft_filter_form", _ptr(fine.wsB), _ptr(V), nb, self.C, int(self.has_clash), L,
                 _ptr(self.W1t), _ptr(self.b1), _ptr(self.W2), self.b2, self.HP, has_clip, clip, self.threshold,
                 aux, C1, int(C1 > 0), tau, ck, cc, cap, self.k3_form, st)
            self._cset_used = cset
            mark("k3_zifft_filter")
        return V[:nb]

    def reset_top(self):
        self.finish()                                   # nothing of the previous pair still in flight
        self.top.exclusion = int(self.exclusion)        # (the radius of THIS search: fixed until the next reset)
        if self.restraints is not self.top.restraints:
            self.top.set_restraints(self.restraints)    # (and its restraint set)
        self.top.reset()

    def select_batch(self, V, nb, cset=None, rot_ids=None):
        """Per-rotation picks of Docker.update_top (Docker.py:89-98) for V (nb, N^3).  cset: the candidate set the
        scoring kernel filled for this batch -- then the rows hold only the picks that can still enter the running list
        (+inf padded) and the cset is consumed; see ``DeviceTopList.select``.  rot_ids: the batch's rotation indices as
        ``merge_batch`` gets them -- needed by a restrained search only."""
        if self.window is not None:
            V = self.gather_window(V, nb)
        return self.top.select(V.reshape(nb, -1), nb, cset, rot_ids)

    def gather_window(self, V, nb):
        """(nb, N^3) scores of this engine's grid -> (nb, (2 extent)^3): the reference's grid of the embedded box."""
        return V.reshape(nb, -1).index_select(1, self.window_flat)

    def merge_batch(self, rot_ids, nb):
        """Docker.py:100-105 on the device-resident list.  rot_ids int32 (nb,) ascending."""
        self.top.merge(rot_ids, nb)

    # ---- two-stream pipeline: top-K of batch i overlaps K1/K2 of batch i+1 -----------------
    def _start_steps(self):
        """step()'s state, made at the first step: a V buffer and a candidate set per slot (two on the device, where
        the side stream consumes one slot while the next batch fills the other; one with the emulated library, which
        runs everything on one stream), the side stream, and per slot the event that frees it and the caller's rot_ids."""
        cuda = self.device.type == "cuda"
        self._Vbuf = [self.V, torch.empty_like(self.V)] if cuda else [self.V]
        self._csets = [self.top.new_candidate_set() if self.prefilter else None for _ in self._Vbuf]
        self._consumed = [None] * len(self._Vbuf)
        self._ids_alive = [None] * len(self._Vbuf)
        self._side = torch.cuda.Stream(device=self.device) if cuda else None
        self._k = 0

    def step(self, R, rot_ids, mark=None, volumes=None, transposed=False, quads=False, occupancy=None):
        """One batch: score on the current stream; select + merge on a side stream (they are
        latency-bound one-block kernels that fit beside the FFT blocks).  V is double-buffered;
        call finish() before reading the list."""
        nb = R.shape[0] if volumes is None else volumes[0].shape[0]
        if self._Vbuf is None:
            self._start_steps()
        if self._side is None:                          # emulated library (tests): same calls, one stream
            V = self.score_batch(R, mark=mark, volumes=volumes, transposed=transposed, quads=quads,
                                 cset=self._csets[0], occupancy=occupancy)
            self.select_batch(V, nb, self._cset_used, rot_ids)
            self.merge_batch(rot_ids, nb)
            return
        k = self._k
        self._k ^= 1
        main = torch.cuda.current_stream(self.device)
        if self._consumed[k] is not None:
            main.wait_event(self._consumed[k])          # V[k] free again
        # (Holding the previous batch's select + merge back until K1 of THIS batch has been issued was measured:
        # K1 -0.06 ms, K2 +0.11 ms -- not kept.)
        V = self.score_batch(R, mark=mark, out=self._Vbuf[k], volumes=volumes, transposed=transposed, quads=quads,
                             cset=self._csets[k], occupancy=occupancy)
        cset = self._cset_used
        self._launch_pending(main)
        # the side stream reads rot_ids later: keep the caller's tensor alive (and its memory out of the
        # allocator's reach) until this buffer slot comes round again
        self._ids_alive[k] = rot_ids
        ready = torch.cuda.Event()
        ready.record(main)
        self._pending = (V, nb, rot_ids, ready, k, cset)
        self._launch_pending(main)

    def _launch_pending(self, main):
        """Enqueue select + merge of the batch that finished last on the side stream: after its scores are
        complete (ready) and after everything issued on the main stream so far."""
        pend, self._pending = self._pending, None
        if pend is None:
            return
        V, nb, rot_ids, ready, k, cset = pend
        gate = torch.cuda.Event()
        gate.record(main)
        with torch.cuda.stream(self._side):
            self._side.wait_event(ready)
            self._side.wait_event(gate)
            self.select_batch(V, nb, cset, rot_ids)
            self.merge_batch(rot_ids, nb)
            done = torch.cuda.Event()
            done.record(self._side)
        self._consumed[k] = done

    def finish(self):
        if self._side is not None:
            main = torch.cuda.current_stream(self.device)
            self._launch_pending(main)
            main.wait_stream(self._side)

    def search(self, R_all, rot_ids=None, progress=None):
        """Score every rotation in R_all (nrot,3,3) and fold it into the running top list.
        rot_ids: global rotation indices (ascending) for this shard; default arange.
        The rotations are visited in groups -- slab orientation (prefers_transposed) x gather layout
        (prefers_quads) -- because both are per-launch choices; the ranked list does not
        depend on the visiting order (merge key = (score, rotation, pick))."""
        dev = self.device
        R_host = torch.as_tensor(R_all).detach().cpu().numpy()
        nrot = R_host.shape[0]
        ids_host = np.arange(nrot) if rot_ids is None else torch.as_tensor(rot_ids).detach().cpu().numpy()
        flags = self.prefers_transposed(R_host) if (self.orient and nrot) else np.zeros(nrot, dtype=bool)
        qflags = self.prefers_quads(R_host) if (self.use_quads and nrot) else np.zeros(nrot, dtype=bool)
        done = 0
        for tr, qd in ((False, False), (False, True), (True, False), (True, True)):
            sel = np.nonzero((flags == tr) & (qflags == qd))[0]
            if len(sel) == 0:
                continue
            R_grp = torch.from_numpy(np.ascontiguousarray(R_host[sel])).to(device=dev, dtype=torch.float32).contiguous()
            ids_grp = torch.from_numpy(np.ascontiguousarray(ids_host[sel]).astype(np.int32)).to(dev)
            for beg in range(0, len(sel), self.batch):
                end = min(beg + self.batch, len(sel))
                self.step(R_grp[beg:end], ids_grp[beg:end], transposed=tr, quads=qd)
                done += end - beg
                if progress is not None:
                    progress(done)
        self.finish()

    # ---- results ------------------------------------------------------------------------
    def top_entries(self):
        self.finish()
        return self.top.entries()

    def top_list(self):
        """[(rotation_index, x, y, z, score)] exactly as Docker.top_list (Docker.py:100-105)."""
        return DeviceTopList.to_top_list(self.top_entries(), self.N)
