"""Exhaustive rotation x translation search driver -- drop-in for the reference's ``Docker``
class (/root/reference/src/Docker/Docker.py:17-238): same constructor, ``new_log``, ``cleanup``,
``update_top``, ``write_conformations``, ``load_batch``, ``dockE3``, ``dockSE3`` and attributes
(``top_list``, ``rot.R``, ``box_size``, ``resolution``, ``box_length``, ``max_conf``, ``log``).

It is constructed and driven exactly as /root/reference/src/local_test.py:55,65-71 does
(``Docker(docking_model=..., angle_inc=..., box_size=80, resolution=1.25, max_conf=2000,
randomize_rot=True)``, ``new_log``, ``dockSE3(rec, lig, batch_size=2)``); every further keyword is
optional.

What differs underneath:
  * the hot loop (Docker.py:211-236) runs in libdlpd.so with no host synchronisation; the clash
    mask, the filter MLP and the mask multiply are fused into the inverse FFT, and the top list
    lives on the device until the pair is finished;
  * the caller's ``batch_size`` does NOT size the launches: the ranked list is independent of how
    the rotations are batched (merge key (score, rotation, pick); tested), so ``dockSE3`` /
    ``dockE3`` always score ``launch_batch`` (32) rotations per launch -- the receptor slab in K2 is
    amortised over the launch batch, and ``batch_size=2`` of local_test.py:69,71 would cost 8x the
    launches;
  * the scoring call ``docking_model(receptor_volumes, ligand_volumes_rotated)`` (Docker.py:229) is
    replaced by the fused kernels only when that is what the model computes -- the reference's
    ``GlobalDockingModel.forward`` with an MLP ``SimpleFilter`` (``Models.fused_filter_parameters``).
    Any other model / filter module is CALLED, on volumes rotated and correlated by the stand-alone
    HIP ops, followed by the device top-K (``_search_unfused``);
  * atoms come from ``Utils.FullAtom.CoordsBackend`` (PDB reader, 11-type typing, GPU density
    projection; TorchProteinLibrary itself is absent, SURVEY.md 8f rows 1,3), created on first use;
    ``coords_backend=`` swaps in another implementation;
  * ``dock_volumes`` is the volume-level entry (a superset): it takes representation volumes
    directly, which is what the synthetic BASELINE configs use;
  * rotations can be sharded over ranks (``rank``/``world_size``): rank r scores rotations
    r, r+W, r+2W, ... and one all-gather of the per-rank top lists + a deterministic merge by
    (score, rotation, pick) reproduces the single-process list.
"""
import atexit
import os

import numpy as np
import torch

from deeplocalproteindocking_amd.engine import DeviceTopList, DockingEngine
from deeplocalproteindocking_amd._lib import get_lib
from deeplocalproteindocking_amd.Utils.Conventions import VolumeConventions
from deeplocalproteindocking_amd.Utils.Rotations import Rotations, euler_to_matrices


def fused_filter_parameters(model):
    from deeplocalproteindocking_amd.Models.DockingModels import fused_filter_parameters as f
    return f(model)


class _PivotRotation(object):
    """ops.VolumeRotation per grid size, with the Docker's rotation conventions (pivot, scale, axis order)."""

    def __init__(self, docker):
        self.docker, self.ops = docker, {}

    def __call__(self, volume, R):
        from deeplocalproteindocking_amd.ops import VolumeRotation
        L = volume.shape[-1]
        if L not in self.ops:
            cv = self.docker.conventions
            self.ops[L] = VolumeRotation(center=self.docker.rotation_pivot(L), lib=self.docker._lib,
                                         scale=cv.rotation_scale, axis_order=cv.rotation_axis_order,
                                         transpose=cv.rotation_transpose)
        return self.ops[L](volume, R)


class _FixedRotations(object):
    def __init__(self, R):
        self.R = torch.as_tensor(np.asarray(R, dtype=np.float64)).reshape(-1, 3, 3)
        self.source = "explicit"


def random_rotation(generator=None, seed=None):
    """Uniform random rotation (1,3,3) float64 -- stand-in for TPL getRandomRotation(1)
    (Docker.py:44); the TPL RNG stream cannot be matched (source absent).
    Without ``generator`` the numbers come from a generator of their own -- seeded with ``seed`` or, for ``None``, from
    the environment variable DLPD_ROTATION_SEED or, for ``None`` and no such variable, from the operating system's
    entropy -- so that the rotation neither repeats from run to run (torch's global generator starts from a fixed default
    seed) nor depends on what else has drawn from the process-global stream."""
    if generator is None:
        if seed is None and os.environ.get("DLPD_ROTATION_SEED", "") != "":
            seed = int(os.environ["DLPD_ROTATION_SEED"])   # an UNCHANGED caller (local_test.py passes no such keyword)
        generator = torch.Generator()
        generator.manual_seed(int(seed)) if seed is not None else generator.seed()
    u = torch.rand(3, generator=generator, dtype=torch.float64).numpy()
    phi, psi = 2 * np.pi * u[0] - np.pi, 2 * np.pi * u[2] - np.pi
    theta = np.arccos(1.0 - 2.0 * u[1])
    return torch.from_numpy(euler_to_matrices(phi, theta, psi)).reshape(1, 3, 3)


def all_gather_top_entries(entries, K, world_size, process_group=None, device="cpu", always=False):
    """The ONE collective of the rotation-sharded search: every rank contributes its local top list
    ``entries`` = (rot, flat index, score, pick) as a fixed-size block, one ``all_gather`` (RCCL over xGMI on the
    ``nccl`` backend, gloo on CPU), then the same deterministic merge on every rank -- sort by (score, rotation, pick),
    keep K -- which reproduces the single-process list exactly: the global top-K is a subset of the union of the
    per-shard top-Ks and the key is the reference's stable insertion order (Docker.py:100-105).
    Used by ``Docker`` and by ``bench.py``'s multi-rank leg alike.  ``always`` runs the collective for a group of one
    too (the one-GPU boxes' RCCL check, scripts/rccl_one_rank_check.py)."""
    if world_size <= 1 and not always:
        return entries
    import torch.distributed as dist
    pack = torch.zeros(4, K + 1, dtype=torch.float64)
    n = len(entries[0])
    pack[0, 0] = n
    pack[0, 1:1 + n] = torch.from_numpy(np.asarray(entries[0], dtype=np.float64))
    pack[1, 1:1 + n] = torch.from_numpy(np.asarray(entries[1], dtype=np.float64))
    score_bits = np.ascontiguousarray(entries[2], dtype=np.float32).view(np.uint32)
    pack[2, 1:1 + n] = torch.from_numpy(score_bits.astype(np.float64))   # exact score bits
    pack[3, 1:1 + n] = torch.from_numpy(np.asarray(entries[3], dtype=np.float64))
    backend = dist.get_backend(process_group)
    buf = pack.to(device) if backend == "nccl" else pack
    out = [torch.empty_like(buf) for _ in range(world_size)]
    dist.all_gather(out, buf, group=process_group)
    parts = []
    for o in out:
        o = o.cpu().numpy()
        m = int(o[0, 0])
        parts.append((o[0, 1:1 + m].astype(np.int64), o[1, 1:1 + m].astype(np.int64),
                      o[2, 1:1 + m].astype(np.uint32).view(np.float32), o[3, 1:1 + m].astype(np.int64)))
    return DeviceTopList.merge_entries(parts, K)


PROVIDER_BATCH_BYTES = 256 << 20      # score_poses: room for the per-pose clash volumes a clash_provider returns at a time
LAUNCH_BATCH = 32      # rotations per launch of the fused pipeline (16 through round 5: EXPERIMENTS.md R6)


class PreparedPair(object):
    """Everything ``dockSE3`` / ``dockE3`` do for a target BEFORE the rotation loop (Docker.py:184-209 / :135-161): the
    two PDB files parsed, typed and centred, the receptor projected and represented, its spectrum in an engine, the
    ligand's volumes (SE3) and its atoms on the device.  ``Docker.prepare`` builds one -- from a host thread of its own if
    the caller wants the next target prepared while the current one is searched (local_test.py sweep), but on the CALLER'S
    stream: device work of a preparation is never put beside a running search (see ``Docker.prepare``) -- and the dock
    call consumes it.  ``ready`` is only set by the diagnostic ``stream=`` form and then orders the consumer's stream
    after the producer's."""

    def __init__(self, group, ureceptor, uligand, slot):
        self.group, self.ureceptor, self.uligand, self.slot = group, ureceptor, uligand, slot
        self.receptor = self.receptor_volumes = self.receptor_forbidden = self.ligand_volumes = None
        self.ligand_atoms = None           # (coords, num_atoms_of_type, offsets) on the device, origin-centred
        self.receptor_shift = self.ligand_shift = None   # the centring shifts load_batch returned: file frame + shift = origin-centred
        self.engine = None                 # fused engine with receptor (and, SE3, ligand) already set; None: other paths
        self.ready = None                  # torch.cuda.Event recorded on the producer's stream
        self.seconds = 0.0                 # host time of the preparation

    def wait(self, device):
        """The caller's current stream waits for the preparation; tensors made on the producer's stream are marked as
        used here so that the caching allocator does not hand their memory out while this stream still reads it."""
        if self.ready is None or device.type != "cuda":
            return
        cur = torch.cuda.current_stream(device)
        cur.wait_event(self.ready)
        for t in self.tensors():
            t.record_stream(cur)

    def tensors(self):
        out = [self.receptor, self.receptor_forbidden] + list(self.receptor_volumes or []) + list(self.ligand_volumes or []) + \
            list(self.ligand_atoms or [])
        return [t for t in out if torch.is_tensor(t) and t.is_cuda]


class Docker:
    def __init__(self, docking_model, angle_inc=15.0, box_size=80, resolution=1.25, max_conf=1000,
                 randomize_rot=False, rotations=None, device="cuda", coords_backend=None,
                 rank=0, world_size=1, process_group=None, lib=None, launch_batch=None, rotation_center=None,
                 conventions=None, rotation_seed=None, collectives_with_one_rank=False, exclusion=0,
                 restraints=None, restraints_needed=None):
        self.docking_model = docking_model
        # Exclusion radius of the search in voxels (BUILD-DEFINED, include/dlpd.h dlpd_topk_suppress; 0 = the reference, which
        # clears one voxel per pick, Docker.py:98): a rotation contributes only the voxels that nothing within `exclusion`
        # voxels (cyclic, Chebyshev) beats.  Settable between searches; dockSE3, dockE3, dock_volumes and update_top honour it.
        self.exclusion = int(exclusion)
        # Distance restraints of the search (BUILD-DEFINED, include/dlpd.h dlpd_topk_restrain; None = the reference): a list of
        # Utils.Restraints.Restraint in the search frame (restraints_from_selections makes them from PDB selections), of which
        # a pose must satisfy restraints_needed (None: all).  Settable between searches; dockSE3, dockE3, dock_volumes and
        # update_top honour them.  Every rank builds the same table from the full rotation set: no collective.
        self.restraints = restraints
        self.restraints_needed = restraints_needed
        self.log = None

        self.box_size = box_size
        self.resolution = resolution
        self.box_length = box_size * resolution

        self.max_conf = max_conf
        self.rot = Rotations(angle_inc=angle_inc) if rotations is None else _FixedRotations(rotations)

        self.box_center = torch.zeros(1, 3, dtype=torch.double, device='cpu')
        self.box_center.fill_(self.box_length / 2.0)

        self.device = torch.device(device)
        self.coords_backend = coords_backend
        self.rank, self.world_size, self.process_group = int(rank), int(world_size), process_group

        # Docker.py:42-45.  Rotation-sharded over ranks, every rank must score the SAME rotated receptor: rank 0's
        # matrix is broadcast (here when the process group already exists, else at the start of the first dock* call);
        # rotation_seed makes it reproducible (None: a fresh one per Docker, as "random" says).
        # collectives_with_one_rank: run the broadcasts and the all-gather for a group of ONE rank too -- how a one-GPU box
        # takes this class through RCCL itself (local_test.py -force_group 1); the results are the same by construction
        self.collectives_with_one_rank = bool(collectives_with_one_rank)
        self.randomize_rot = randomize_rot
        self._randR_shared = self.world_size <= 1 and not self.collectives_with_one_rank
        if self.randomize_rot:
            self.randR = random_rotation(seed=rotation_seed)
            self._share_random_rotation(required=False)
            if self.rank == 0 or not self._randR_shared:
                print("Adding random rotation to the receptor:", self.randR)
        self._lib = lib
        self.launch_batch = int(launch_batch or os.environ.get("DLPD_LAUNCH_BATCH", LAUNCH_BATCH))
        # Pivot of the trilinear VOLUME rotation in voxel-index units (build-defined: TorchProteinLibrary's
        # VolumeRotation has no source here).  None: index L/2 of each grid (the box centre when voxel i spans
        # [i, i+1) * resolution, Docker.py:221-223); "grid_sample": (L-1)/2 of each grid (the centre of
        # torch's align_corners=False sampling grid); a number: that index on the fine grid, scaled to coarser ones.
        # conventions: a Utils.Conventions.VolumeConventions (or the path of the JSON scripts/calibrate_tpl.py writes): the
        # remaining build-defined choices -- rotation scale and axis order, what VolumeConvolution(clip) clamps, the
        # density splat -- next to the pivot.  ``rotation_center`` given explicitly wins over the file's.
        if isinstance(conventions, str):
            conventions = VolumeConventions.load(conventions)
        # (a copy: the rotation_center setter below must not reach into an object the caller shares between Dockers)
        self.conventions = conventions.copy() if conventions is not None else VolumeConventions()
        if rotation_center is not None:
            self.conventions = VolumeConventions.from_dict(dict(self.conventions.to_dict(), rotation_center=rotation_center))
        self._ops_cache = {}
        # box sizes without a compiled plan: on the fused kernels inside the next compiled box (_search_plan);
        # False: the plan-free stand-alone ops (ops.VolumeConvolution._forward_generic), any box up to 128
        self.embed_uncompiled_boxes = True
        # dockE3 on the fused engine: a plugin with occupancy maps does not write the tiles it skips (the engine goes by the
        # maps); False: every voxel of the batch's volumes is written (same lists; DLPD_UNWRITTEN_ACTIVATIONS=0)
        self.unwritten_activations = os.environ.get("DLPD_UNWRITTEN_ACTIVATIONS", "1") != "0"
        # the search side's occupancy maps (DockingEngine(sparse_k1=)): None = decided per ligand; DLPD_K1_OCCUPANCY=0 / 1 forces
        # the dense / the map kernels for whole programs (A/B runs: the lists are the same either way)
        self.k1_occupancy = {"0": False, "1": True}.get(os.environ.get("DLPD_K1_OCCUPANCY", ""))
        self._top = None            # DeviceTopList behind update_top()
        self.top_list = []
        self.engine = None
        self._engine_pool = {}      # slot -> (key, engine): slot 1 exists only while targets are prepared ahead (prepare)
        atexit.register(self.cleanup)

    def _share_random_rotation(self, required=True):
        """world_size > 1: replace this rank's ``randR`` by rank 0's (one broadcast of nine doubles, once per Docker).
        Without it the ranks would score differently rotated receptors and merge them into one silently wrong list."""
        if not self.randomize_rot or self._randR_shared:
            return
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            if required:
                raise Exception("Docker(world_size=%d, randomize_rot=True) needs an initialised torch.distributed "
                                "process group to share the random rotation" % self.world_size)
            return
        group = self.process_group
        src = dist.get_global_rank(group, 0) if group is not None else 0
        buf = self.randR.to(dtype=torch.float64).reshape(9).clone()
        if dist.get_backend(group) == "nccl":
            buf = buf.to(self.device)
        dist.broadcast(buf, src=src, group=group)
        self.randR = buf.cpu().reshape(1, 3, 3)
        self._randR_shared = True

    # ------------------------------------------------------------------ the reference's operator objects
    # Docker.py:29-40 creates TorchProteinLibrary operators as attributes; nothing outside the class reads them, but
    # a subclass may.  They are thin views of the coords backend / the volume ops with TPL's call signatures,
    # created on first use (the constructor must not need a GPU or a backend).
    @property
    def rotate(self):                       # CoordsRotate()(coords, R, num_atoms)
        return self._need_backend().rotate

    @property
    def translate(self):                    # CoordsTranslate()(coords, T, num_atoms)
        return self._need_backend().translate

    translation = translate

    @property
    def pdb2coords(self):                   # PDB2CoordsUnordered()(filenames)
        return self._need_backend().pdb2coords

    @property
    def assignTypes(self):                  # Coords2TypedCoords()(coords, resnames, atomnames, num_atoms)
        return self._need_backend().assign_types

    @property
    def project(self):                      # TypedCoords2Volume(box_size, resolution)(coords, num_atoms_of_type, offsets)
        be = self._need_backend()
        return lambda coords, num_atoms_of_type, offsets: be.project(coords, num_atoms_of_type, offsets, self.box_size,
                                                                     self.resolution, self.device)

    @property
    def convolve(self):                     # VolumeConvolution()(volume1, volume2): no clip (Docker.py:32)
        from deeplocalproteindocking_amd.ops import VolumeConvolution
        key = ("convolve", self.embed_uncompiled_boxes)
        if key not in self._ops_cache:      # one object per Docker, as the reference's attribute is
            self._ops_cache[key] = VolumeConvolution(lib=self._lib, embed=self.embed_uncompiled_boxes)
        return self._ops_cache[key]

    @property
    def vol_rotate(self):                   # VolumeRotation()(volume, R), with this Docker's rotation conventions
        if "vol_rotate" not in self._ops_cache:
            self._ops_cache["vol_rotate"] = _PivotRotation(self)
        return self._ops_cache["vol_rotate"]

    # ------------------------------------------------------------------ logging (Docker.py:63-84)
    def new_log(self, log_file_name, rewrite=True):
        """Open the .dat of the next target.  Resume rule of Docker.py:63-79: with ``rewrite=False`` a file
        that already holds more than one non-blank line counts as finished -- no log is opened and False is
        returned so the caller skips the target; anything else is (re)started from scratch."""
        self.cleanup()
        if not rewrite and self.log_is_complete(log_file_name):
            return False
        self.log = open(log_file_name, "w")
        return True

    @staticmethod
    def log_is_complete(log_file_name):
        """The test of the resume rule alone (Docker.py:66-76), without opening anything: does the file exist and hold
        more than one non-blank line?  (A sweep uses it to decide which target to prepare ahead.)"""
        if not os.path.exists(log_file_name):
            return False
        with open(log_file_name) as existing:
            return sum(1 for line in existing if line.split()) > 1

    def cleanup(self):
        """Close the current log, if any (also registered with atexit, Docker.py:46,81-84)."""
        log, self.log = self.log, None
        if log is not None:
            log.close()

    # ------------------------------------------------------------------ top list (Docker.py:86-105)
    def _library(self):
        if self._lib is None:
            self._lib = get_lib()
        return self._lib

    def restraint_table(self):
        """The integer table of ``self.restraints`` over this Docker's whole rotation set (None without restraints); built once
        per (restraints, restraints_needed) object pair."""
        if not self.restraints:
            return None
        key = (tuple((r.receptor_point.tobytes(), r.ligand_point.tobytes(), r.dmax, r.dmin) for r in self.restraints),
               self.restraints_needed, float(self.resolution))
        if getattr(self, "_rst_table", (None, None))[0] != key:
            from deeplocalproteindocking_amd.Utils.Restraints import restraint_table
            self._rst_table = (key, restraint_table(self.rot.R, self.restraints, self.resolution, self.restraints_needed))
        return self._rst_table[1]

    def restraints_from_selections(self, prepared, selections):
        """[(receptor selection, ligand selection, dmax[, dmin]), ...] -- "CHAIN:RESNUM[:ATOM]" in the two PDB files of
        ``prepared`` (Utils.Restraints.select_point) -> [Restraint] in the search frame: the receptor point becomes
        randR (x + shift), the ligand point x + shift, with the centring shifts the pair was prepared with."""
        from deeplocalproteindocking_amd.Utils.Restraints import Restraint, select_point
        rsh = np.asarray(torch.as_tensor(prepared.receptor_shift).detach().cpu(), dtype=np.float64).reshape(3)
        lsh = np.asarray(torch.as_tensor(prepared.ligand_shift).detach().cpu(), dtype=np.float64).reshape(3)
        randR = self.randR.squeeze().to(torch.float64).cpu().numpy() if self.randomize_rot else np.eye(3)
        out = []
        for sel in selections:
            rec_sel, lig_sel, dmax = sel[0], sel[1], sel[2]
            dmin = sel[3] if len(sel) > 3 else 0.0
            b = randR @ (select_point(prepared.ureceptor, rec_sel) + rsh)
            a = select_point(prepared.uligand, lig_sel) + lsh
            out.append(Restraint(b, a, dmax, dmin))
        return out

    def restraint_report(self, poses=None):
        """Number of ``self.restraints`` each pose satisfies -> int array (default: ``self.top_list``; any list form of
        ``_pose_arrays``; the fractional translations of a ``refined_list`` are taken as they stand).  Host side.  Entries of a
        ``top_list`` go by their rotation index and the search's own integer test; other forms by their own rotation matrix."""
        from deeplocalproteindocking_amd.Utils.Restraints import restraint_table, satisfied
        poses = self.top_list if poses is None else poses
        if not self.restraints:
            raise RuntimeError("dlpd: restraint_report without restraints")
        if len(poses) == 0:
            return np.zeros(0, dtype=np.int64)
        R, t, own, _ = self._pose_arrays(poses)
        if all(len(e) == 5 for e in poses):
            return satisfied(self.restraint_table(), np.array([int(e[0]) for e in poses]), np.array(own, dtype=np.int64).reshape(-1, 3))
        tab = restraint_table(R, self.restraints, self.resolution, self.restraints_needed)
        return satisfied(tab, np.arange(len(poses)), t)

    def update_top(self, V, rotation_index):
        """V (N,N,N) float32 device tensor.  Same observable behaviour as Docker.py:86-105: the
        max_conf picks are appended to ``self.top_list`` (stable sort, truncate) and the picked
        voxels of V are set to 0.0 in place.  The list is kept on the device; ``self.top_list``
        is refreshed from it."""
        if self._top is None or self._top.K != self.max_conf or self._top.device != V.device:
            self._top = DeviceTopList(self.max_conf, 1, V.device, self._library())
            self._top.reset()
        elif len(self.top_list) == 0:
            self._top.reset()                      # caller cleared top_list: a new pair starts
        Vc = V.contiguous()
        self._top.exclusion = int(self.exclusion)  # (> 0: the picks of suppress_r(V); V itself loses the picked voxels only)
        tab = self.restraint_table()
        if tab is not self._top.restraints:
            self._top.set_restraints(tab)
        rid = torch.tensor([rotation_index], dtype=torch.int32, device=V.device)
        _, idx = self._top.select(Vc.reshape(1, -1), 1, None, rid)
        self._top.merge(rid, 1)
        Vc.view(-1)[idx[0].long()] = 0.0           # Docker.py:98, V is mutated in place
        if Vc.data_ptr() != V.data_ptr():
            V.copy_(Vc)
        self.top_list = DeviceTopList.to_top_list(self._top.entries(), V.shape[0])

    # ------------------------------------------------------------------ output (Docker.py:107-133)
    def write_conformations(self):
        """One line per pose: the 9 entries of R row-major, the translation in Angstrom, the score -- 13
        tab-separated ``%f`` columns (Docker.py:107-133, byte-exact against fixture G4).  Grid indices at
        or beyond ``box_size`` are negative shifts (index - 2L); with ``randomize_rot`` both R and t are
        taken back to the receptor's original frame by randR^T."""
        if self.log is None:
            return
        L, N = self.box_size, 2 * self.box_size
        undo = self.randR.squeeze().t().to(torch.double) if self.randomize_rot else None
        rows = []
        for rot_index, x, y, z, score in self.top_list:
            r = self.rot.R[rot_index].to(torch.double)
            shift = torch.tensor([v - N if v >= L else v for v in (x, y, z)], dtype=torch.double)
            t = shift * self.resolution
            if undo is not None:
                t, r = undo @ t, undo @ r
            cols = [float(v) for v in r.reshape(-1)] + [float(v) for v in t] + [score]
            rows.append("\t".join("%f" % v for v in cols))
        if rows:
            self.log.write("\n".join(rows) + "\n")
        self.log.flush()

    # ------------------------------------------------------------------ local docking: given poses (csrc/dlpd_local.h)
    def score_poses(self, receptor_volumes, ligand_volumes, R, T, receptor_forbidden=None, ligand_forbidden=None,
                    clash_provider=None, radius=0, shift=None):
        """Scores of GIVEN poses by direct correlation: (P, W, W, W) float32 on ``self.device``, W = 2 radius + 1; entry
        [p, dx, dy, dz] is the pose (R[p], T[p] + (dx, dy, dz) - radius).  R (P, 3, 3) rotation matrices, T (P, 3) signed integer
        translations in fine-grid voxels, |t| < box_size.  The GLOBAL search's conventions throughout -- this Docker's rotation
        conventions, the model's clip and clash threshold, floor(t / 2) on the coarse grid -- so a pose of ``top_list`` gets the
        score the search gave it: ``score_poses(rot.R[i], signed (x, y, z))[0, 0, 0, 0]``.  The volumes and the clash
        arguments are ``dock_volumes``'s.  Poses are processed in batches sized from the kernel's workspace.
        ``shift`` (P, 3) float, fine-grid voxels: a fraction of a voxel added to ``T`` -- the ligand is resampled at the displaced
        position inside the correlation's own trilinear gather (csrc/dlpd_rotate_shift.h).  The coarse resolution gets
        ``shift / scale`` on top of its floor(t / scale), and a stored ``ligand_forbidden`` is displaced the same way.  With a
        ``clash_provider`` the clash mask is taken at the WHOLE-voxel translation ``T``: the provider's signature has no
        translation, its volumes cannot be displaced by a fraction.  Zeros give the bits of the call without ``shift``."""
        model = self.docking_model
        if receptor_forbidden is not None and ligand_forbidden is None and clash_provider is None:
            raise Exception("score_poses: receptor_forbidden needs the ligand's side of the clash channel: ligand_forbidden or clash_provider")
        # the model is scored in eval mode and handed back in the mode it came in (a scoring call inside a training loop)
        was_training = bool(getattr(model, "training", False))
        if was_training:
            model.eval()
        try:
            return self._score_poses(receptor_volumes, ligand_volumes, R, T, receptor_forbidden, ligand_forbidden, clash_provider, radius,
                                     shift)
        finally:
            if was_training:
                model.train()

    def _pose_inputs(self, receptor_volumes, ligand_volumes, receptor_forbidden, ligand_forbidden, clash_provider):
        """What scoring given poses needs on the device, by the search's conventions: the volumes per resolution, fine / coarse
        edge, the clip the features take, the forbidden volumes (rf; lf None with a provider)."""
        model = self.docking_model
        dev = self.device
        rec = [torch.as_tensor(v, dtype=torch.float32) for v in receptor_volumes]
        lig = [torch.as_tensor(v, dtype=torch.float32) for v in ligand_volumes]
        rec = [v.reshape((-1,) + tuple(v.shape[-3:])).to(dev).contiguous() for v in rec]
        lig = [v.reshape((-1,) + tuple(v.shape[-3:])).to(dev).contiguous() for v in lig]
        L = rec[0].shape[-1]
        if L != self.box_size:
            raise Exception("Volume size does not match box_size", L, self.box_size)
        scale = 1
        if len(rec) == 2:
            scale = L // rec[1].shape[-1]
        if len(rec) > 2 or (len(rec) == 2 and (scale not in (1, 2) or rec[1].shape[-1] * scale != L)):
            raise Exception("score_poses: one resolution, or two with the coarser at the same or half the edge")
        cv = self.conventions
        clip = getattr(model, "clip", 5.0) if cv.clip_mode != "none" else None
        if clip is not None and cv.clip_mode == "input":
            rec, lig = [v.clamp(-float(clip), float(clip)) for v in rec], [v.clamp(-float(clip), float(clip)) for v in lig]
            clip = None
        rf = lf = None
        if receptor_forbidden is not None:
            rf = torch.as_tensor(receptor_forbidden, dtype=torch.float32).reshape(1, L, L, L).to(dev).contiguous()
            if clash_provider is None:
                lf = torch.as_tensor(ligand_forbidden, dtype=torch.float32).reshape(1, L, L, L).to(dev).contiguous()
        return rec, lig, scale, clip, rf, lf

    def _score_poses(self, receptor_volumes, ligand_volumes, R, T, receptor_forbidden, ligand_forbidden, clash_provider, radius,
                     shift=None):
        from deeplocalproteindocking_amd import ops
        model = self.docking_model
        dev, lib = self.device, self._lib
        cv = self.conventions
        rec, lig, scale, clip, rf, lf = self._pose_inputs(receptor_volumes, ligand_volumes, receptor_forbidden, ligand_forbidden,
                                                          clash_provider)
        L = rec[0].shape[-1]
        R = torch.as_tensor(np.asarray(R, dtype=np.float64) if not torch.is_tensor(R) else R).reshape(-1, 3, 3)
        T = torch.as_tensor(np.asarray(T) if not torch.is_tensor(T) else T).reshape(-1, 3)
        P, r = R.shape[0], int(radius)
        if T.shape[0] != P:
            raise Exception("score_poses: one translation per rotation", T.shape[0], P)
        Td = T.to(torch.int32).to(dev).contiguous()
        Rf = R.to(device=dev, dtype=torch.float32).contiguous()
        Sf = None
        if shift is not None:
            Sf = torch.as_tensor(np.asarray(shift, dtype=np.float64) if not torch.is_tensor(shift) else shift).reshape(-1, 3)
            if Sf.shape[0] != P:
                raise Exception("score_poses: one shift per pose", Sf.shape[0], P)
            Sf = Sf.to(device=dev, dtype=torch.float32).contiguous()
        has_clash = rf is not None
        params = fused_filter_parameters(model)
        W = 2 * r + 1
        out = torch.empty(P, W, W, W, dtype=torch.float32, device=dev)
        # batches: the provider's re-projected clash volumes are L^3 floats per pose
        batch = max(1, min(P, PROVIDER_BATCH_BYTES // (4 * L ** 3))) if (has_clash and clash_provider is not None) else P
        for beg in range(0, P, batch):
            sl = slice(beg, min(P, beg + batch))
            Rb, Tb = Rf[sl], Td[sl]
            Sb = None if Sf is None else Sf[sl]
            corr0 = ops.local_correlate(rec[0], lig[0], Tb, R=cv.matrices(Rb, L), radius=r, scale=1, coarse="floor",
                                        center=self.rotation_pivot(L), lib=lib, shift=Sb)
            corr1 = None
            if len(rec) == 2:
                L1 = rec[1].shape[-1]
                corr1 = ops.local_correlate(rec[1], lig[1], Tb, R=cv.matrices(Rb, L1), radius=ops.local_coarse_radius(r, scale), scale=scale,
                                            coarse="floor", center=self.rotation_pivot(L1), lib=lib,
                                            shift=None if Sb is None else Sb / float(scale))
            clash = None
            if has_clash:
                if clash_provider is not None:
                    lfb = clash_provider(Rb).reshape(Rb.shape[0], 1, L, L, L).contiguous()
                    clash = ops.local_correlate(rf, lfb, Tb, R=None, radius=r, lib=lib)
                else:
                    clash = ops.local_correlate(rf, lf, Tb, R=cv.matrices(Rb, L), radius=r, center=self.rotation_pivot(L), lib=lib,
                                                shift=Sb)
                clash = clash.reshape(Rb.shape[0], W, W, W)
            res = None
            if params is not None:
                W1, b1, W2, b2 = params
                res = ops.local_filter(corr0, corr1, clash, Tb, r, W1, b1, W2, b2, scale=scale, coarse="floor", clip=clip,
                                       threshold=getattr(model, "threshold_clash", 0.0), lib=lib)
            if res is not None:
                out[sl] = res[0]
            else:                                   # any other filter module is CALLED on the features
                feat = ops.local_features(corr0, corr1, Tb, r, scale=scale, coarse="floor", clip=clip)
                with torch.no_grad():
                    V = model.filter(feat).reshape(Rb.shape[0], W, W, W).to(torch.float32)
                if clash is not None:
                    V = torch.lt(clash, model.threshold_clash).to(torch.float32) * V
                out[sl] = V
        return out

    def signed_translation(self, x, y, z):
        """Grid indices of the (2 box_size)^3 score volume -> signed shifts (Docker.py:115-120)."""
        L, N = self.box_size, 2 * self.box_size
        return tuple(int(v) - N if int(v) >= L else int(v) for v in (x, y, z))

    def refine(self, receptor_volumes, ligand_volumes, receptor_forbidden=None, ligand_forbidden=None, clash_provider=None,
               poses=None, perturbations=None, radius=1):
        """Local refinement of a list of poses (default: ``self.top_list``, which is not touched): for pose
        (i, x, y, z, score) and every Q of ``perturbations`` ((n, 3, 3); default ``local_perturbations(5, 1)``) the rotation
        Q @ rot.R[i] is scored over the (2 radius + 1)^3 window round the pose's signed translation (``score_poses``) and the
        best (Q, d) is kept -- the first Q and the lowest window index on a tie.  -> ``self.refined_list``: entries
        (R float64 (3, 3), (tx, ty, tz) signed ints, score, position of the source pose in ``poses``), stable-sorted by score.
        With the identity among the perturbations an entry is never worse than its re-scored source pose.
        Every rank refines the whole (gathered) list; there is no collective here."""
        from deeplocalproteindocking_amd.Utils.Rotations import local_perturbations
        poses = list(self.top_list if poses is None else poses)
        Q = local_perturbations(5.0, 1) if perturbations is None else perturbations
        Q = torch.as_tensor(np.asarray(Q, dtype=np.float64) if not torch.is_tensor(Q) else Q).to(torch.float64).reshape(-1, 3, 3)
        nq, npose, W = Q.shape[0], len(poses), 2 * int(radius) + 1
        self.refined_list = []
        if npose == 0:
            return self.refined_list
        base = torch.stack([self.rot.R[int(p[0])].to(torch.float64) for p in poses])           # (npose, 3, 3)
        Rall = torch.matmul(Q[None], base[:, None])                                             # (npose, nq, 3, 3)
        t = torch.tensor([self.signed_translation(p[1], p[2], p[3]) for p in poses], dtype=torch.int32)
        Tall = t[:, None, :].expand(-1, nq, -1)
        S = self.score_poses(receptor_volumes, ligand_volumes, Rall.reshape(-1, 3, 3), Tall.reshape(-1, 3), receptor_forbidden,
                             ligand_forbidden, clash_provider, radius=radius)
        S = S.reshape(npose, nq * W ** 3).cpu().numpy()
        pick = np.argmin(S, axis=1)                          # first occurrence of the minimum: lowest (Q, d)
        r = int(radius)
        for n in range(npose):
            q, d = divmod(int(pick[n]), W ** 3)
            dx, dy, dz = d // (W * W) - r, (d // W) % W - r, d % W - r
            tt = (int(t[n, 0]) + dx, int(t[n, 1]) + dy, int(t[n, 2]) + dz)
            self.refined_list.append((Rall[n, q].numpy().copy(), tt, float(S[n, pick[n]]), n))
        self.refined_list.sort(key=lambda e: e[2])
        return self.refined_list

    def write_refined_conformations(self):
        """``self.refined_list`` in the format of ``write_conformations`` (13 tab-separated ``%f`` columns, the matrix taken
        from the entry, ``randomize_rot`` undone the same way): Results.DockerParser reads it unchanged."""
        if self.log is None:
            return
        undo = self.randR.squeeze().t().to(torch.double) if self.randomize_rot else None
        rows = []
        for R, tt, score, _ in getattr(self, "refined_list", []):
            r = torch.as_tensor(R, dtype=torch.double)
            t = torch.tensor(tt, dtype=torch.double) * self.resolution
            if undo is not None:
                t, r = undo @ t, undo @ r
            cols = [float(v) for v in r.reshape(-1)] + [float(v) for v in t] + [score]
            rows.append("\t".join("%f" % v for v in cols))
        if rows:
            self.log.write("\n".join(rows) + "\n")
        self.log.flush()

    # ------------------------------------------------------------------ pose clustering (csrc/dlpd_cluster.h; build-defined)
    def _pose_arrays(self, poses):
        """Entries of either list form -> (R (K, 3, 3) float64, t (K, 3) float64 in voxels, the entries' own translations,
        scores): ``top_list`` entries (rot, x, y, z, score) through ``signed_translation``, ``refined_list`` entries
        (R, (tx, ty, tz), score, src) as they stand (fractions of a voxel included)."""
        R, t, own, score = [], [], [], []
        for e in poses:
            if len(e) == 5:
                R.append(self.rot.R[int(e[0])].detach().cpu().to(torch.float64).numpy())
                own.append(self.signed_translation(e[1], e[2], e[3]))
                score.append(float(e[4]))
            else:
                R.append(np.array(e[0], dtype=np.float64).reshape(3, 3))
                own.append(tuple(e[1]))
                score.append(float(e[2]))
            t.append([float(v) for v in own[-1]])
        return np.stack(R), np.array(t, dtype=np.float64).reshape(-1, 3), own, score

    def cluster(self, ligand_coords, poses=None, radius=None, keep=None, weights=None, rank="score"):
        """Greedy clustering of a list of poses by the RMSD between them (default: ``self.top_list``; a ``refined_list`` is
        taken too; neither is touched).  ``ligand_coords`` (n, 3): the ligand's atoms in Angstrom, centred on the origin as
        the search holds them (``PreparedPair.ligand_atoms``); pose p carries atom x to R_p x + t_p, t_p the entry's
        translation times ``resolution``; ``weights`` (n) >= 0 select or weigh atoms (C-alpha only, a fixed subset).  In list
        order (best score first) a pose is a centre iff no earlier centre lies within ``radius`` Angstrom of it (required:
        there is no default), every other pose joins the first such centre.  ``keep``: at most that many clusters.
        ``rank="size"`` re-sorts the clusters by population (stable: equal sizes keep their score order) before ``keep``
        cuts.  The list is clustered in the search frame -- a rigid motion common to all poses changes no distance -- and
        ``randomize_rot`` is undone by the writer alone.
        -> ``self.clustered_list``: entries (R float64 (3, 3), the centre's translation in voxels, score, position of the centre
        in ``poses``, size of the cluster), and ``self.cluster_labels`` (len(poses)) int32: the entry of ``clustered_list``
        each pose belongs to, -1 for a pose none of the kept clusters covers.  At most 65,536 poses.
        Every rank clusters the same (gathered) list; there is no collective here."""
        from deeplocalproteindocking_amd import ops
        if radius is None or not float(radius) >= 0.0:
            raise Exception("cluster needs a radius in Angstrom (>= 0); there is no default", radius)
        if rank not in ("score", "size"):
            raise Exception("Unknown cluster ranking", rank)
        if keep is not None and int(keep) <= 0:
            raise Exception("cluster keep must be positive", keep)
        poses = list(self.top_list if poses is None else poses)
        self.clustered_list, self.cluster_labels = [], np.zeros(0, dtype=np.int32)
        if not poses:
            return self.clustered_list
        R, t, own, score = self._pose_arrays(poses)
        coords = ligand_coords.detach().cpu().numpy() if torch.is_tensor(ligand_coords) else np.asarray(ligand_coords)
        E, _ = ops.pose_embedding(coords.reshape(-1, 3), R, t * float(self.resolution), weights, device=self.device)
        first = None if rank == "size" or keep is None else int(keep)
        centres, sizes, labels = ops.pose_cluster(E, float(radius), max_clusters=first, lib=self._lib)
        centres, sizes, labels = centres.cpu().numpy(), sizes.cpu().numpy(), labels.cpu().numpy()
        order = np.arange(len(centres))
        if rank == "size":
            order = np.argsort(-sizes.astype(np.int64), kind="stable")
            if keep is not None:
                order = order[:int(keep)]
            place = np.full(len(centres) + 1, -1, dtype=np.int32)          # (the last slot: label -1 stays -1)
            place[order] = np.arange(len(order), dtype=np.int32)
            labels = place[labels]
        self.clustered_list = [(R[c].copy(), own[c], score[c], int(c), int(sizes[n])) for n, c in ((n, int(centres[n])) for n in order)]
        self.cluster_labels = labels.astype(np.int32)
        return self.clustered_list

    def cluster_prepared(self, prepared, poses=None, radius=None, keep=None, weights=None, rank="score"):
        """``cluster`` with the ligand's atoms taken from the ``PreparedPair`` the search ran on (origin-centred, on the device)."""
        lc, ln, _ = prepared.ligand_atoms
        n = int(ln.sum())
        return self.cluster(lc.reshape(-1)[:3 * n].reshape(n, 3), poses=poses, radius=radius, keep=keep, weights=weights, rank=rank)

    def write_clustered_conformations(self):
        """The centres of ``self.clustered_list`` in the format of ``write_conformations`` (13 tab-separated ``%f`` columns,
        ``randomize_rot`` undone the same way): Results.DockerParser reads it unchanged."""
        if self.log is None:
            return
        undo = self.randR.squeeze().t().to(torch.double) if self.randomize_rot else None
        rows = []
        for R, tt, score, _, _ in getattr(self, "clustered_list", []):
            r = torch.as_tensor(R, dtype=torch.double)
            t = torch.tensor(tt, dtype=torch.double) * self.resolution
            if undo is not None:
                t, r = undo @ t, undo @ r
            cols = [float(v) for v in r.reshape(-1)] + [float(v) for v in t] + [score]
            rows.append("\t".join("%f" % v for v in cols))
        if rows:
            self.log.write("\n".join(rows) + "\n")
        self.log.flush()

    # ------------------------------------------------------------------ evaluation against a native (csrc/dlpd_evaluate.h)
    def dat_frame_poses(self, poses):
        """Entries of ``top_list``, ``refined_list`` or ``clustered_list`` -> (K, 12) float64, R row-major then t in Angstrom, in
        the frame of the .dat file: what ``write_conformations`` / ``write_refined_conformations`` /
        ``write_clustered_conformations`` put on a line before ``%f`` rounds it (``randomize_rot`` undone by randR^T on both R
        and t).  A ``clustered_list`` entry has five fields as a ``top_list`` entry has: the forms are told apart by the first
        field, a rotation index or a matrix."""
        undo = self.randR.squeeze().t().to(torch.double).numpy() if self.randomize_rot else None
        out = np.zeros((len(poses), 12), dtype=np.float64)
        for k, e in enumerate(poses):
            if np.ndim(e[0]) == 0:
                r = self.rot.R[int(e[0])].detach().cpu().to(torch.float64).numpy()
                t = np.array(self.signed_translation(e[1], e[2], e[3]), dtype=np.float64)
            else:
                r = np.array(e[0], dtype=np.float64).reshape(3, 3)
                t = np.array([float(v) for v in e[1]], dtype=np.float64)
            t = t * float(self.resolution)
            if undo is not None:
                t, r = undo @ t, undo @ r
            out[k, :9], out[k, 9:] = r.reshape(-1), t
        return out

    def evaluate(self, native, poses=None, fnonnat=False):
        """How good every pose of a list is (default: ``self.top_list``; ``refined_list`` and ``clustered_list`` entries are
        taken too; none of the lists is touched): ``native`` is a ``Results.InterfaceSelection.NativeReference`` of the target
        (``native_reference`` of the bound and unbound files).  -> ``self.evaluation``, a dict of numpy arrays aligned with
        the poses: ``irmsd`` and ``lrmsd`` in Angstrom, ``fnat`` (float64) and ``capri`` (int32, 0 incorrect .. 3 high).
        ``fnonnat``: also ``fnonnat`` (float64, the share of the pose's residue contacts the native does not have), ``n_dec``
        and ``n_corr`` (int32, ops.pose_contact_counts); ``native`` must then have been built with ``all_contacts=True``.
        At most 65,536 poses.  Every rank evaluates the same (gathered) list; there is no collective here."""
        from deeplocalproteindocking_amd import ops
        poses = list(self.top_list if poses is None else poses)
        self.evaluation = {"irmsd": np.zeros(0), "lrmsd": np.zeros(0), "fnat": np.zeros(0), "capri": np.zeros(0, dtype=np.int32)}
        if fnonnat:
            if getattr(native, "all", None) is None:
                raise RuntimeError("dlpd: Docker.evaluate(fnonnat=True) needs a native reference built with all_contacts=True")
            self.evaluation.update({"fnonnat": np.zeros(0), "n_dec": np.zeros(0, dtype=np.int32), "n_corr": np.zeros(0, dtype=np.int32)})
        if not poses:
            return self.evaluation
        P = self.dat_frame_poses(poses)
        got = ops.pose_evaluate(P, native.to(self.device), lib=self._lib)
        self.evaluation = {k: v.cpu().numpy() for k, v in zip(("irmsd", "lrmsd", "fnat", "capri"), got)}
        if fnonnat:
            n_dec, n_corr = ops.pose_contact_counts(P, native, lib=self._lib)
            self.evaluation.update({"fnonnat": ops.fnonnat_of(n_dec, n_corr).cpu().numpy(), "n_dec": n_dec.cpu().numpy(),
                                    "n_corr": n_corr.cpu().numpy()})
        return self.evaluation

    def write_evaluation(self):
        """``self.evaluation`` into the open log, one line per pose: irmsd, lrmsd, fnat (``%f``) and the class, tab-separated;
        an evaluation that carries ``fnonnat`` writes it (``%f``) as a fifth column"""
        if self.log is None:
            return
        ev = getattr(self, "evaluation", None)
        if ev is not None and len(ev["capri"]):
            if "fnonnat" in ev:
                self.log.write("\n".join("%f\t%f\t%f\t%d\t%f" % (i, l, f, c, g) for i, l, f, c, g in
                                         zip(ev["irmsd"], ev["lrmsd"], ev["fnat"], ev["capri"], ev["fnonnat"])) + "\n")
            else:
                self.log.write("\n".join("%f\t%f\t%f\t%d" % (i, l, f, c) for i, l, f, c in
                                         zip(ev["irmsd"], ev["lrmsd"], ev["fnat"], ev["capri"])) + "\n")
        self.log.flush()

    # ------------------------------------------------------------------ interface consensus (csrc/dlpd_interface.h; build-defined)
    @staticmethod
    def _complex_residues(complex):
        rr, lr = getattr(complex, "rec_residues", None), getattr(complex, "lig_residues", None)
        if getattr(complex, "all", None) is None or rr is None or lr is None:
            raise RuntimeError("dlpd: the interface steps need a ComplexReference (Results.InterfaceSelection.complex_reference) or a "
                               "native reference built with all_contacts=True")
        return list(rr), list(lr)

    def _interface_weights(self, poses, weights, temperature):
        """-> float64 weights of the poses on the host (the doc of ``interface``)"""
        K = len(poses)
        if isinstance(weights, str):
            if weights == "uniform":
                return np.full(K, 1.0 / K, dtype=np.float64)
            if weights == "rank":
                w = 1.0 / (1.0 + np.arange(K, dtype=np.float64))
                return w / w.sum()
            if weights == "boltzmann":
                if temperature is None or not float(temperature) > 0.0:
                    raise Exception("boltzmann weights need a temperature > 0", temperature)
                s = np.array([float(e[4]) if np.ndim(e[0]) == 0 else float(e[2]) for e in poses], dtype=np.float64)
                w = np.exp(-(s - s.min()) / float(temperature))
                return w / w.sum()
            raise Exception("Unknown interface weights", weights)
        w = np.asarray(weights.detach().cpu().numpy() if torch.is_tensor(weights) else weights, dtype=np.float64).reshape(-1)
        if len(w) != K:
            raise Exception("interface weights must be one number per pose", len(w), K)
        return w

    def _interface_bits_of(self, complex, poses):
        """the residue bitmaps of ``poses``; those of the last ``interface`` call are reused for the same list object"""
        from deeplocalproteindocking_amd import ops
        held = getattr(self, "_interface_of", None)
        if held is not None and held[0] is poses and held[1] is complex and len(poses) == held[2]:
            return self.interface_bits
        if len(poses) > ops.POSE_CLUSTER_MAX:
            raise RuntimeError("dlpd: the interface steps take at most %d poses, got %d" % (ops.POSE_CLUSTER_MAX, len(poses)))
        complex.to(self.device)
        P = self.dat_frame_poses(poses)
        self.interface_bits = ops.pose_interface_bits(P, complex, float(complex.contact_dist), lib=self._lib)
        self._interface_of = (poses, complex, len(poses))
        return self.interface_bits

    def interface(self, complex, poses=None, weights="uniform", temperature=None):
        """Which residues of each protein a list of poses puts in the interface (default: ``self.top_list``; ``refined_list``
        and ``clustered_list`` entries are taken too; none of the lists is touched).  ``complex``: a ``ComplexReference`` of the
        two unbound files (Results.InterfaceSelection.complex_reference), or a native reference built with
        ``all_contacts=True``.  A residue is in a pose's interface iff one of its atoms lies within ``complex.contact_dist`` of
        an atom of the partner.  ``weights``: "uniform" (1 / K each); "boltzmann": exp(-(s - s_min) / ``temperature``)
        normalised to sum 1 (``temperature`` required, in the units of the score); "rank": 1 / (1 + position) normalised;
        or K numbers taken as they are -- float64 on the host in every case.
        -> ``self.interface_profile``, a dict of numpy arrays ``rec_freq`` / ``lig_freq`` (float64: the summed weights of the
        poses that mark a residue), ``rec_count`` / ``lig_count`` (int32: their number), with ``rec_residues`` /
        ``lig_residues`` ((chain, resnum, name), in the arrays' order) and ``K``; and ``self.interface_bits``, the two bitmaps
        on the device (ops.pose_interface_bits; ops.unpack_bits for host filters).  An empty list gives empty bitmaps and zeros
        without a launch.  At most 65,536 poses.  Every rank treats the same (gathered) list; there is no collective here."""
        from deeplocalproteindocking_amd import ops
        poses = self.top_list if poses is None else poses
        rr, lr = self._complex_residues(complex)
        self._interface_of = None
        bits = self._interface_bits_of(complex, poses)
        w = self._interface_weights(poses, weights, temperature) if len(poses) else None
        got = ops.interface_profile(bits[0], bits[1], len(rr), len(lr), w, lib=self._lib)
        self.interface_profile = {k: v.cpu().numpy() for k, v in zip(("rec_freq", "lig_freq", "rec_count", "lig_count"), got)}
        self.interface_profile.update({"rec_residues": rr, "lig_residues": lr, "K": len(poses)})
        return self.interface_profile

    def interface_residues(self, side, n=None, min_freq=None):
        """The residues of one side ("receptor" / "ligand", or "R" / "L") of ``self.interface_profile`` that some pose marks,
        sorted by falling frequency, ties in file order; ``n``: at most that many; ``min_freq``: only those at or above it.
        -> "CHAIN:RESNUM" strings ("_" for a blank chain), the selections ``restraints_from_selections`` takes."""
        prof = getattr(self, "interface_profile", None)
        if not isinstance(prof, dict):
            raise RuntimeError("dlpd: interface_residues needs Docker.interface first")
        key = {"receptor": "rec", "r": "rec", "rec": "rec", "ligand": "lig", "l": "lig", "lig": "lig"}.get(str(side).lower())
        if key is None:
            raise Exception("Unknown side", side)
        freq, count, residues = prof[key + "_freq"], prof[key + "_count"], prof[key + "_residues"]
        order = [int(i) for i in np.argsort(-freq, kind="stable") if count[i] > 0 and (min_freq is None or freq[i] >= float(min_freq))]
        if n is not None:
            order = order[:int(n)]
        return ["%s:%d" % (residues[i][0] if str(residues[i][0]).strip() else "_", residues[i][1]) for i in order]

    def cluster_interface(self, complex, poses=None, threshold=None, keep=None, rank="score"):
        """``cluster`` with the similarity of two poses' interfaces in place of the RMSD between them: poses i and j are
        neighbours iff the residue sets they put in the interface (both proteins' together) have a Jaccard index
        |A & B| / |A | B| >= ``threshold`` (in [0, 1], required: there is no default; compared as the integer
        round(1024 threshold)); two poses without an interface are neighbours.  Same greedy scan in list order, same ``keep``
        and ``rank``, same ``self.clustered_list`` / ``self.cluster_labels``: the writer, ``evaluate`` and ``refine`` take the
        result unchanged.  The bitmaps of ``self.interface_bits`` are reused when ``interface`` was run on the same list
        object and complex."""
        from deeplocalproteindocking_amd import ops
        if threshold is None or not 0.0 <= float(threshold) <= 1.0:
            raise Exception("cluster_interface needs a threshold in [0, 1] (a Jaccard index); there is no default", threshold)
        if rank not in ("score", "size"):
            raise Exception("Unknown cluster ranking", rank)
        if keep is not None and int(keep) <= 0:
            raise Exception("cluster keep must be positive", keep)
        poses = self.top_list if poses is None else poses
        self._complex_residues(complex)
        self.clustered_list, self.cluster_labels = [], np.zeros(0, dtype=np.int32)
        if not len(poses):
            return self.clustered_list
        bits = self._interface_bits_of(complex, poses)
        R, _, own, score = self._pose_arrays([e[:4] if (len(e) == 5 and np.ndim(e[0]) != 0) else e for e in poses])
        first = None if rank == "size" or keep is None else int(keep)
        centres, sizes, labels = ops.interface_cluster(bits[0], bits[1], float(threshold), max_clusters=first, lib=self._lib)
        centres, sizes, labels = centres.cpu().numpy(), sizes.cpu().numpy(), labels.cpu().numpy()
        order = np.arange(len(centres))
        if rank == "size":
            order = np.argsort(-sizes.astype(np.int64), kind="stable")
            if keep is not None:
                order = order[:int(keep)]
            place = np.full(len(centres) + 1, -1, dtype=np.int32)          # (the last slot: label -1 stays -1)
            place[order] = np.arange(len(order), dtype=np.int32)
            labels = place[labels]
        self.clustered_list = [(R[c].copy(), own[c], score[c], int(c), int(sizes[n])) for n, c in ((n, int(centres[n])) for n in order)]
        self.cluster_labels = labels.astype(np.int32)
        return self.clustered_list

    def write_interface(self):
        """``self.interface_profile`` into the open log, one line per residue that some pose marks: R or L, chain, residue number,
        name, count, frequency (``%f``), tab-separated; the receptor's residues first, each side in file order"""
        if self.log is None:
            return
        prof = getattr(self, "interface_profile", None)
        rows = []
        if isinstance(prof, dict):
            for tag, key in (("R", "rec"), ("L", "lig")):
                for res, c, f in zip(prof[key + "_residues"], prof[key + "_count"], prof[key + "_freq"]):
                    if c > 0:
                        rows.append("%s\t%s\t%d\t%s\t%d\t%f" % (tag, res[0], res[1], res[2], c, f))
        if rows:
            self.log.write("\n".join(rows) + "\n")
        self.log.flush()

    def refine_prepared(self, prepared, perturbations=None, radius=1, poses=None):
        """``refine`` for a target given as files: the ``PreparedPair`` the SE3 search ran on (``prepare`` / ``dockSE3``) holds
        the volumes; the clash channel is re-projected from the rotated ligand atoms as ``dockSE3`` does (Docker.py:221-224)."""
        if prepared.group != "SE3":
            raise Exception("refine needs the ligand's volumes: SE3 pairs only", prepared.group)
        be = self._need_backend()
        L, res, dev = self.box_size, self.resolution, self.device
        lc, ln, lo = prepared.ligand_atoms
        with torch.no_grad():
            def provider(Rb):
                return be.project(lc, ln, lo, L, res, dev, R=Rb, shift=self.box_center, sum_types=True)
            return self.refine(prepared.receptor_volumes, prepared.ligand_volumes, prepared.receptor_forbidden, None,
                               clash_provider=provider, poses=poses, perturbations=perturbations, radius=radius)

    # ------------------------------------------------------------------ descent in the pose itself (csrc/dlpd_rotate_rgrad.h)
    @staticmethod
    def _rodrigues(omega):
        """exp([omega]x) for omega (n, 3) float64, differentiable at omega = 0 too (the series of sin t / t and
        (1 - cos t) / t^2 below |omega|^2 = 1e-12)."""
        t2 = (omega * omega).sum(dim=1)
        small = t2 < 1e-12
        t = torch.sqrt(torch.where(small, torch.ones_like(t2), t2))
        A = torch.where(small, 1.0 - t2 / 6.0, torch.sin(t) / t)
        B = torch.where(small, 0.5 - t2 / 24.0, (1.0 - torch.cos(t)) / (t * t))
        z = torch.zeros_like(t2)
        K = torch.stack([z, -omega[:, 2], omega[:, 1], omega[:, 2], z, -omega[:, 0], -omega[:, 1], omega[:, 0], z], dim=1).reshape(-1, 3, 3)
        eye = torch.eye(3, dtype=omega.dtype).expand_as(K)
        return eye + A[:, None, None] * K + B[:, None, None] * torch.matmul(K, K)

    def _pose_objective(self, inputs, clash_provider, base, omega, T, radius, shift=None):
        """Score of the states (exp([omega]x) base, T): the minimum of the (2 radius + 1)^3 window of ``_score_poses``'
        scores -- the same conventions, the correlations from ``ops.local_correlate_rotated(rotation_grad=True)``, the filter
        CALLED on ``ops.local_features``, the clash mask a constant 0 / 1 factor -- its flat window index (the lowest on a tie)
        and the gradient of that entry with respect to omega.  -> (score (n), index (n), gradient (n, 3)), float64 on the CPU.
        ``shift`` (n, 3) float64, fine-grid voxels (``minimize(translation=True)``): the states are (exp([omega]x) base, T + shift),
        and a fourth result is the gradient of the same entry with respect to ``shift``."""
        from deeplocalproteindocking_amd import ops
        model, cv, dev, lib = self.docking_model, self.conventions, self.device, self._lib
        rec, lig, scale, clip, rf, lf = inputs
        L, r, n = rec[0].shape[-1], int(radius), omega.shape[0]
        W = 2 * r + 1
        batch = max(1, min(n, PROVIDER_BATCH_BYTES // (4 * L ** 3))) if (rf is not None and clash_provider is not None) else n
        score, index, grad, gshift = [], [], [], []
        for beg in range(0, n, batch):
            sl = slice(beg, min(n, beg + batch))
            w = omega[sl].detach().clone().requires_grad_()
            sv = None if shift is None else shift[sl].detach().clone().requires_grad_()
            with torch.enable_grad():
                Rb = torch.matmul(self._rodrigues(w), base[sl]).to(device=dev, dtype=torch.float32)
                Tb = T[sl].to(torch.int32).to(dev).contiguous()
                Sb = None if sv is None else sv.to(device=dev, dtype=torch.float32)
                corr0 = ops.local_correlate_rotated(rec[0], lig[0], Tb, cv.matrices(Rb, L), radius=r, scale=1, coarse="floor",
                                                    center=self.rotation_pivot(L), lib=lib, rotation_grad=True, shift=Sb)
                corr1 = None
                if len(rec) == 2:
                    L1 = rec[1].shape[-1]
                    corr1 = ops.local_correlate_rotated(rec[1], lig[1], Tb, cv.matrices(Rb, L1), radius=ops.local_coarse_radius(r, scale),
                                                        scale=scale, coarse="floor", center=self.rotation_pivot(L1), lib=lib,
                                                        rotation_grad=True, shift=None if Sb is None else Sb / float(scale))
                feat = ops.local_features(corr0, corr1, Tb, r, scale=scale, coarse="floor", clip=clip)
                V = model.filter(feat).reshape(Rb.shape[0], W ** 3).to(torch.float32)
                if rf is not None:
                    with torch.no_grad():
                        Rd = Rb.detach().contiguous()
                        if clash_provider is not None:
                            lfb = clash_provider(Rd).reshape(Rd.shape[0], 1, L, L, L).contiguous()
                            clash = ops.local_correlate(rf, lfb, Tb, R=None, radius=r, lib=lib)
                        else:
                            clash = ops.local_correlate(rf, lf, Tb, R=cv.matrices(Rd, L), radius=r, center=self.rotation_pivot(L), lib=lib,
                                                        shift=None if Sb is None else Sb.detach())
                        mask = torch.lt(clash.reshape(Rd.shape[0], W ** 3), model.threshold_clash).to(torch.float32)
                    V = mask * V
                Vd = V.detach()
                low = Vd.min(dim=1, keepdim=True).values
                ar = torch.arange(W ** 3, device=dev).expand_as(Vd)
                idx = torch.where(Vd == low, ar, torch.full_like(ar, W ** 3)).min(dim=1).values          # the lowest index on a tie
                picked = V.gather(1, idx[:, None])
                if sv is None:
                    (g,) = torch.autograd.grad(picked.sum(), w, allow_unused=True)      # (through that entry only; no parameter's .grad)
                else:
                    g, gs = torch.autograd.grad(picked.sum(), (w, sv), allow_unused=True)
                    gshift.append(torch.zeros_like(sv) if gs is None else gs.detach())
            score.append(picked.detach().reshape(-1).to("cpu", torch.float64))
            index.append(idx.to("cpu"))
            grad.append(torch.zeros_like(w) if g is None else g.detach())
        if shift is not None:
            return torch.cat(score), torch.cat(index), torch.cat(grad), torch.cat(gshift)
        return torch.cat(score), torch.cat(index), torch.cat(grad)

    def minimize(self, receptor_volumes, ligand_volumes, receptor_forbidden=None, ligand_forbidden=None, clash_provider=None,
                 poses=None, radius=1, steps=20, max_angle=2.0, min_angle=0.02, translation=False, lever=None):
        """Descent of the score in the rotation itself, for a list of poses (default: ``self.top_list``, which is not touched).
        Pose (i, x, y, z, score) starts at R0 = rot.R[i] and its signed translation; the state is omega (3, float64, from 0), the
        rotation exp([omega]x) R0.  The score of a state is the minimum of the (2 radius + 1)^3 window of ``score_poses``'
        scores round the state's translation (the lowest index on a tie), the translation is recentred on that entry, and the
        gradient is taken through that entry (``ops.local_correlate_rotated(rotation_grad=True)``; the clash mask is a constant
        factor).  Per pose: alpha = ``max_angle`` degrees; the trial omega - alpha g / |g| is accepted only if its score is
        strictly lower, otherwise alpha halves; a pose stops after ``steps`` trials, when alpha < ``min_angle`` or when
        |g| = 0 (a fully masked window).  All poses advance together; nothing is random.
        -> ``self.refined_list`` in ``refine``'s format: (R float64 (3, 3), (tx, ty, tz) signed ints, score, position of the source
        pose in ``poses``), stable-sorted by score; the scores are ``score_poses``' at the final pose, and a pose whose descent
        did not end strictly below its re-scored source comes back as that source.  Every rank minimises the whole list.
        ``translation=True``: a rigid-body descent -- the state is (omega, s), s (3, float64, from 0) a FRACTION of a fine-grid voxel
        added to the translation (``score_poses(shift=)``; csrc/dlpd_rotate_shift.h), and the gradient is taken through the picked
        window entry with respect to both.  Steps are taken in the scaled coordinates (lever * omega, s), ``lever`` in voxels
        (default box_size / 4: a rotation by theta counts as lever * theta voxels): the trial step has length alpha * lever along
        the normalised scaled gradient; accept / halve / stop as above.  After an accepted step the whole voxels of s move into
        the integer translation (s stays in [-0.5, 0.5]).  Entries carry the translation as three FLOATS T + s, which
        ``split_translation`` takes apart again, and the scores are ``score_poses(R, T, shift=s)``' own.  With a ``clash_provider``
        the mask is the whole-voxel one (``score_poses``).  ``translation=False`` is the descent above, ints included."""
        if translation:
            return self._minimize_rigid(receptor_volumes, ligand_volumes, receptor_forbidden, ligand_forbidden, clash_provider, poses,
                                        radius, steps, max_angle, min_angle, lever)
        if receptor_forbidden is not None and ligand_forbidden is None and clash_provider is None:
            raise Exception("minimize: receptor_forbidden needs the ligand's side of the clash channel: ligand_forbidden or clash_provider")
        poses = list(self.top_list if poses is None else poses)
        self.refined_list = []
        if len(poses) == 0:
            return self.refined_list
        model = self.docking_model
        was_training = bool(getattr(model, "training", False))
        if was_training:
            model.eval()
        try:
            r, W, n = int(radius), 2 * int(radius) + 1, len(poses)
            inputs = self._pose_inputs(receptor_volumes, ligand_volumes, receptor_forbidden, ligand_forbidden, clash_provider)
            base = torch.stack([self.rot.R[int(p[0])].to(torch.float64) for p in poses]).cpu()                 # (n, 3, 3)
            t0 = torch.tensor([self.signed_translation(p[1], p[2], p[3]) for p in poses], dtype=torch.int64)

            def window_offset(idx):
                return torch.stack([idx // (W * W) - r, (idx // W) % W - r, idx % W - r], dim=1)
            omega = torch.zeros(n, 3, dtype=torch.float64)
            f, idx, g = self._pose_objective(inputs, clash_provider, base, omega, t0, r)
            T = t0 + window_offset(idx)
            alpha = torch.full((n,), float(np.deg2rad(max_angle)), dtype=torch.float64)
            floor_, left = float(np.deg2rad(min_angle)), torch.full((n,), int(steps), dtype=torch.int64)
            while True:
                norm = g.norm(dim=1)
                act = torch.nonzero((left > 0) & (alpha >= floor_) & (norm > 0)).reshape(-1)
                if act.numel() == 0:
                    break
                trial = omega[act] - (alpha[act] / norm[act])[:, None] * g[act]
                ft, it, gt = self._pose_objective(inputs, clash_provider, base[act], trial, T[act], r)
                ok = ft < f[act]
                won, lost = act[ok], act[~ok]
                omega[won], f[won], g[won] = trial[ok], ft[ok], gt[ok]
                T[won] = T[won] + window_offset(it[ok])
                alpha[lost] = alpha[lost] * 0.5
                left[act] -= 1
            with torch.no_grad():
                Rfin = torch.matmul(self._rodrigues(omega), base)
            both = self._score_poses(receptor_volumes, ligand_volumes, torch.cat([base, Rfin]), torch.cat([t0, T]), receptor_forbidden,
                                     ligand_forbidden, clash_provider, 0).reshape(2, n).cpu().numpy()
        finally:
            if was_training:
                model.train()
        for k in range(n):
            if both[1, k] < both[0, k]:
                self.refined_list.append((Rfin[k].numpy().copy(), tuple(int(v) for v in T[k]), float(both[1, k]), k))
            else:
                self.refined_list.append((base[k].numpy().copy(), tuple(int(v) for v in t0[k]), float(both[0, k]), k))
        self.refined_list.sort(key=lambda e: e[2])
        return self.refined_list

    @staticmethod
    def split_translation(tt):
        """A translation of ``minimize(translation=True)``'s list, three floats -> (the whole voxels T = floor(t + 1/2) as ints,
        the fractions s = t - T in [-0.5, 0.5) as floats): the (T, shift) ``score_poses`` takes.  The subtraction is exact in
        float64, so the split of a list entry is the split its score was computed with."""
        T = [int(np.floor(float(v) + 0.5)) for v in tt]
        return tuple(T), tuple(float(v) - k for v, k in zip(tt, T))

    def _minimize_rigid(self, receptor_volumes, ligand_volumes, receptor_forbidden, ligand_forbidden, clash_provider, poses, radius,
                        steps, max_angle, min_angle, lever):
        """``minimize(translation=True)`` (its docstring)."""
        if receptor_forbidden is not None and ligand_forbidden is None and clash_provider is None:
            raise Exception("minimize: receptor_forbidden needs the ligand's side of the clash channel: ligand_forbidden or clash_provider")
        poses = list(self.top_list if poses is None else poses)
        self.refined_list = []
        if len(poses) == 0:
            return self.refined_list
        lever = float(self.box_size) / 4.0 if lever is None else float(lever)
        if not lever > 0:
            raise Exception("minimize: lever must be positive (voxels)", lever)
        model = self.docking_model
        was_training = bool(getattr(model, "training", False))
        if was_training:
            model.eval()
        try:
            r, W, n = int(radius), 2 * int(radius) + 1, len(poses)
            inputs = self._pose_inputs(receptor_volumes, ligand_volumes, receptor_forbidden, ligand_forbidden, clash_provider)
            base = torch.stack([self.rot.R[int(p[0])].to(torch.float64) for p in poses]).cpu()                 # (n, 3, 3)
            t0 = torch.tensor([self.signed_translation(p[1], p[2], p[3]) for p in poses], dtype=torch.int64)

            def window_offset(idx):
                return torch.stack([idx // (W * W) - r, (idx // W) % W - r, idx % W - r], dim=1)
            omega, s = torch.zeros(n, 3, dtype=torch.float64), torch.zeros(n, 3, dtype=torch.float64)
            f, idx, g, gs = self._pose_objective(inputs, clash_provider, base, omega, t0, r, shift=s)
            T = t0 + window_offset(idx)
            alpha = torch.full((n,), float(np.deg2rad(max_angle)), dtype=torch.float64)
            floor_, left = float(np.deg2rad(min_angle)), torch.full((n,), int(steps), dtype=torch.int64)
            while True:
                # the gradient in the scaled coordinates (lever * omega, s)
                norm = torch.sqrt((g * g).sum(dim=1) / lever ** 2 + (gs * gs).sum(dim=1))
                act = torch.nonzero((left > 0) & (alpha >= floor_) & (norm > 0)).reshape(-1)
                if act.numel() == 0:
                    break
                step = (alpha[act] * lever / norm[act])[:, None]                        # a step of length alpha * lever (voxels)
                trial_w = omega[act] - step * g[act] / lever ** 2
                trial_s = s[act] - step * gs[act]
                ft, it, gt, gst = self._pose_objective(inputs, clash_provider, base[act], trial_w, T[act], r, shift=trial_s)
                ok = ft < f[act]
                won, lost = act[ok], act[~ok]
                omega[won], f[won], g[won], gs[won] = trial_w[ok], ft[ok], gt[ok], gst[ok]
                whole = torch.floor(trial_s[ok] + 0.5)                                  # whole voxels of s move into T
                s[won] = trial_s[ok] - whole
                T[won] = T[won] + window_offset(it[ok]) + whole.to(torch.int64)
                alpha[lost] = alpha[lost] * 0.5
                left[act] -= 1
            with torch.no_grad():
                Rfin = torch.matmul(self._rodrigues(omega), base)
            # the list's translation is T + s as floats; its score is that of the split split_translation returns
            tt = (T.to(torch.float64) + s).numpy()
            split = [self.split_translation(row) for row in tt]
            Tn = torch.tensor([k for k, _ in split], dtype=torch.int64).reshape(n, 3)
            sn = torch.tensor([q for _, q in split], dtype=torch.float64).reshape(n, 3)
            both = self._score_poses(receptor_volumes, ligand_volumes, torch.cat([base, Rfin]), torch.cat([t0, Tn]), receptor_forbidden,
                                     ligand_forbidden, clash_provider, 0, shift=torch.cat([torch.zeros_like(sn), sn]))
            both = both.reshape(2, n).cpu().numpy()
        finally:
            if was_training:
                model.train()
        for k in range(n):
            if both[1, k] < both[0, k]:
                self.refined_list.append((Rfin[k].numpy().copy(), tuple(float(v) for v in tt[k]), float(both[1, k]), k))
            else:
                self.refined_list.append((base[k].numpy().copy(), tuple(float(v) for v in t0[k]), float(both[0, k]), k))
        self.refined_list.sort(key=lambda e: e[2])
        return self.refined_list

    def minimize_prepared(self, prepared, radius=1, poses=None, steps=20, max_angle=2.0, min_angle=0.02, translation=False, lever=None):
        """``minimize`` for a target given as files, as ``refine_prepared``: the SE3 ``PreparedPair``'s volumes, the clash channel
        re-projected from the rotated ligand atoms (with ``translation=True``: at the whole-voxel translation)."""
        if prepared.group != "SE3":
            raise Exception("minimize needs the ligand's volumes: SE3 pairs only", prepared.group)
        be = self._need_backend()
        L, res, dev = self.box_size, self.resolution, self.device
        lc, ln, lo = prepared.ligand_atoms

        def provider(Rb):
            with torch.no_grad():
                return be.project(lc, ln, lo, L, res, dev, R=Rb, shift=self.box_center, sum_types=True)
        return self.minimize(prepared.receptor_volumes, prepared.ligand_volumes, prepared.receptor_forbidden, None,
                             clash_provider=provider, poses=poses, radius=radius, steps=steps, max_angle=max_angle,
                             min_angle=min_angle, translation=translation, lever=lever)

    @property
    def rotation_center(self):
        return self.conventions.rotation_center

    @rotation_center.setter
    def rotation_center(self, value):
        self.conventions.rotation_center = value
        self._ops_cache.pop("vol_rotate", None)          # (its per-size operators carry the pivot)

    def rotation_pivot(self, L):
        """Pivot index of the volume rotation on a grid of L voxels per edge (see ``rotation_center``)."""
        return self.conventions.pivot(L, self.box_size)

    def release_engine(self):
        """Drop the cached fused engine and its device workspaces (several GB at box 80: wsB for 32 rotations,
        double-buffered score volumes).  The next ``dock*`` call builds a new one."""
        for _, eng in self._engine_pool.values():
            eng.finish()
        self._engine_pool = {}
        self.engine, self._engine_key = None, None
        self._top = None

    # ------------------------------------------------------------------ the search on volumes
    def shard(self, nrot):
        """Rotation indices of this rank: interleaved, ascending."""
        return np.arange(self.rank, nrot, self.world_size, dtype=np.int64)

    def dock_volumes(self, receptor_volumes, ligand_volumes, receptor_forbidden=None, ligand_forbidden=None,
                     batch_size=None, rot_indices=None, write=True, clash_provider=None, model_batch=None, prepared=None):
        """Search all rotations for one pair given its representation volumes.

        receptor_volumes / ligand_volumes: lists of (1,C_i,L_i,L_i,L_i) (or (C_i,L_i,..)) tensors
        as returned by ``docking_model.representation``; *_forbidden: (L,L,L)-shaped clash
        densities (``None`` -> no clash exclusion).  The ligand forbidden volume is rotated with
        the same trilinear kernel as the representation unless ``clash_provider`` re-projects it
        from rotated atoms (Docker.py:221-224).
        batch_size: rotations per launch (None -> ``self.launch_batch``); the list does not depend
        on it.  model_batch: rotations per call of a model that has to be CALLED (generic path)."""
        model = self.docking_model
        model.eval() if hasattr(model, "eval") else None
        self._share_random_rotation()           # (write_conformations undoes randR: the same matrix on every rank)
        rec = [torch.as_tensor(v, dtype=torch.float32) for v in receptor_volumes]
        lig = [torch.as_tensor(v, dtype=torch.float32) for v in ligand_volumes]
        rec = [v.reshape((-1,) + tuple(v.shape[-3:])) for v in rec]
        lig = [v.reshape((-1,) + tuple(v.shape[-3:])) for v in lig]
        L = rec[0].shape[-1]
        if L != self.box_size:
            raise Exception("Volume size does not match box_size", L, self.box_size)
        nb = int(batch_size or self.launch_batch)
        R_all = self.rot.R
        ids = self.shard(R_all.shape[0]) if rot_indices is None else np.asarray(rot_indices, dtype=np.int64)
        params = fused_filter_parameters(model)
        if receptor_forbidden is None:          # no clash exclusion: the ligand's side of the channel is never read
            ligand_forbidden = clash_provider = None
        # prepared: a PreparedPair whose engine already holds this receptor's spectrum and this ligand (Docker.prepare)
        pre_eng = prepared.engine if prepared is not None else None
        path, eng, Lc = self._search_plan(rec, receptor_forbidden, params, nb, pre_eng)
        if eng is not None:
            if pre_eng is None:
                # (embedded: the volumes in the corner of the Lc^3 box, the batch's re-projected clash volumes likewise)
                fit = (lambda v, s=1: self._embed(torch.as_tensor(v, dtype=torch.float32), Lc // s)) if Lc else (lambda v, s=1: v)
                lf = ligand_forbidden if ligand_forbidden is not None else torch.zeros(L, L, L)
                eng.set_ligand(fit(lig[0]), fit(torch.as_tensor(lf).reshape(L, L, L)), fit(lig[1], 2) if eng.C1 > 0 else None)
            eng.clash_provider = clash_provider
            if Lc and clash_provider is not None:
                forb_e = torch.zeros(nb, Lc, Lc, Lc, dtype=torch.float32, device=self.device)

                def provider(Rb):          # (Docker.py:221-224)
                    n = Rb.shape[0]
                    forb_e[:n, :L, :L, :L] = clash_provider(Rb).reshape(n, L, L, L)
                    return forb_e[:n]
                eng.clash_provider = provider
            eng.reset_top()
            eng.search(R_all[ids], rot_ids=ids)          # (embedded: the engine's top-K works on the gathered (2L)^3 grid)
            entries = eng.top_entries()
            if Lc:
                eng.clash_provider = None                # (it holds the Lc^3 buffers)
        else:
            entries = self._search_unfused(path, rec, receptor_forbidden, ids, nb if path == "ops" else int(model_batch or nb),
                                           self._rotated_ligand(lig, ligand_forbidden, clash_provider), params)
        entries = self._gather(entries)
        self.top_list = DeviceTopList.to_top_list(entries, 2 * L)
        if write:
            self.write_conformations()
        return self.top_list

    def _make_engine(self, rec, receptor_forbidden, batch_size, params, inner_box=None, slot=0):
        """DockingEngine for one receptor (one resolution, or the reference's [C0 @ L, C1 @ L/2] pair);
        None when the fused pipeline has no kernel for the shape (other grids or resolution layouts,
        hidden width above 32) or the model's scoring is not the MLP it fuses: the stand-alone-op paths
        take over."""
        if params is None:
            return None
        lib = self._library()
        L = rec[0].shape[-1]
        if not lib.call("dlpd_grid_supported", int(L)):
            return None
        two_res = len(rec) == 2 and rec[1].shape[-1] * 2 == L and bool(lib.call("dlpd_grid_supported", L // 2))
        if not (len(rec) == 1 or two_res):
            return None
        W1, b1, W2, b2 = params
        HP = int(lib.call("dlpd_fused_hidden_pad", int(W1.shape[0]), int(L), int(two_res)))
        if HP < 0 or W1.shape[1] != sum(v.shape[0] for v in rec):
            return None
        model = self.docking_model
        # one engine (multi-GB workspaces, side stream, top-list buffers) serves every pair of the same shape:
        # local_test.py docks hundreds of targets with one Docker
        C, C1, has_clash = rec[0].shape[0], (rec[1].shape[0] if two_res else 0), receptor_forbidden is not None
        # inner_box: the volumes are inner_box^3 boxes in the corner of the L^3 ones (_search_plan): pivots and
        # crop of the rotation are the small box's
        Lp = int(inner_box or L)
        cv = self.conventions
        if cv.clip_mode == "input" and Lp < L:
            return None          # clamped INPUTS are not combined with embedded boxes: the stand-alone ops take the pair
        key = (int(L), int(C), int(C1), has_clash, HP, int(self.max_conf),
               int(batch_size), str(self.device), self.rotation_pivot(Lp), Lp, cv.scale(Lp), cv.rotation_axis_order, cv.clip_mode,
               cv.rotation_transpose)
        pooled = self._engine_pool.get(slot)
        eng = pooled[1] if pooled is not None and pooled[0] == key else None
        if eng is None:
            eng = DockingEngine(L, C, W1.cpu(), b1.cpu(), W2.cpu(), b2.cpu(), clip=getattr(model, "clip", 5.0),
                                threshold_clash=model.threshold_clash, has_clash=has_clash, max_conf=self.max_conf,
                                batch=batch_size, device=self.device, lib=self._lib, coarse_channels=C1,
                                center=self.rotation_pivot(Lp), coarse_center=self.rotation_pivot(Lp // 2),
                                extent=(Lp if Lp < L else None), rotation_scale=cv.scale(Lp),
                                coarse_rotation_scale=cv.scale(Lp // 2), rotation_axis_order=cv.rotation_axis_order,
                                clip_mode=cv.clip_mode, rotation_transpose=cv.rotation_transpose, sparse_k1=self.k1_occupancy)
            self._engine_pool[slot] = (key, eng)
        else:
            eng.finish()
            eng.set_filter(W1.cpu(), b1.cpu(), W2.cpu(), b2.cpu())
            eng.clip, eng.threshold = getattr(model, "clip", 5.0), float(model.threshold_clash)
        eng.set_receptor(rec[0], receptor_forbidden, rec[1] if two_res else None)
        eng.holds_pair = None                            # (prepare() names the PreparedPair this content belongs to)
        if slot == 0:
            self.engine, self._engine_key = eng, key
        return eng

    @staticmethod
    def _embed(v, Le):
        """v (..., l, l, l) in the corner of a zero (..., Le, Le, Le) volume."""
        out = torch.zeros(tuple(v.shape[:-3]) + (Le, Le, Le), dtype=torch.float32, device=v.device)
        l = v.shape[-1]
        out[..., :l, :l, :l] = v
        return out

    def _embedding_box(self, L, two_res):
        """The smallest box WITH a compiled plan that holds an L^3 volume (and, for the reference's two
        resolutions, whose half holds the L/2 grid); None if there is none."""
        lib = self._library()
        for Lc in (32, 40, 64, 80):
            if Lc > L and lib.call("dlpd_grid_supported", Lc):
                if not two_res or (L % 2 == 0 and lib.call("dlpd_grid_supported", Lc // 2)):
                    return Lc
        return None

    def _search_plan(self, rec, receptor_forbidden, params, nb, prepared_engine=None):
        """Which code searches this receptor -> (path, eng, Lc); the one writer of ``self.path``, ``self.engine_box`` and, for a
        pooled engine, ``self.engine``.
          fused     ``DockingEngine`` on the box's own compiled plan (``prepared_engine``, or ``_make_engine``): eng, Lc None;
          embedded  the same engine on the next compiled box Lc, the volumes in its corner (below): eng, Lc;
          ops       the stand-alone ops + the HIP filter kernel (``_ops_path_ok``): eng None;
          call      the model really called, whatever module it is: eng None.
        embedded -- a box size without a compiled plan on the FUSED kernels (box_size is a free argument of the reference,
        Docker.py:18,22-24,31): the L^3 volumes sit in the corner of the next compiled box Lc^3, zeros around them.
        The correlation of two L-sized volumes is linear for every translation |t| < L on any grid of at least 2L
        points, so the 2Lc grid holds the reference's (2L)^3 grid exactly: index t for 0 <= t <= L (t = L: no overlap,
        zero -- the reference's wrap plane) and 2Lc + t for -L < t < 0.  The engine rotates the embedded ligand about the
        SMALL box's pivot and crops the result to the small box (K1's ``extent``, include/dlpd.h), so a batch costs what
        it costs at box Lc; the scores of the reference's grid are gathered out of the larger one -- monotonic in every
        index, so ties keep the reference's order -- for the device top-K.  Taken with ``embed_uncompiled_boxes`` when the
        model's scoring is the fused MLP, over one resolution or the L, L/2 pair, and a compiled box fits."""
        L = rec[0].shape[-1]
        eng, Lc = prepared_engine, None
        if eng is None:
            eng = self._make_engine(rec, receptor_forbidden, nb, params)
        two_res = len(rec) == 2 and rec[1].shape[-1] * 2 == L
        if eng is None and params is not None and self.embed_uncompiled_boxes and (len(rec) == 1 or two_res) and \
                not self._library().call("dlpd_grid_supported", int(L)):
            Lc = self._embedding_box(L, two_res)
            if Lc is not None:
                rf = receptor_forbidden
                if rf is not None:
                    rf = self._embed(torch.as_tensor(rf, dtype=torch.float32).reshape(L, L, L), Lc)
                eng = self._make_engine([self._embed(rec[0], Lc)] + ([self._embed(rec[1], Lc // 2)] if two_res else []), rf, nb,
                                        params, inner_box=L)
                Lc = Lc if eng is not None else None
        if eng is not None:
            self.path, self.engine = ("embedded" if Lc else "fused"), eng
            eng.exclusion = int(self.exclusion)          # (read by the reset_top() that starts the search)
            eng.restraints = self.restraint_table()
        else:
            self.path = "ops" if self._ops_path_ok(rec, params) else "call"
        self.engine_box = Lc
        return self.path, eng, Lc

    @staticmethod
    def _ops_path_ok(rec, params):
        """The stand-alone ops + the HIP per-voxel filter kernel cover an MLP filter of hidden width
        <= 64 over one or two resolutions (dlpd_filter_mask)."""
        return params is not None and params[0].shape[0] <= 64 and len(rec) <= 2

    def _convolutions(self):
        """-> (convolve, conv_noclip) of the unfused paths: the model's own correlation -- the reference's op with its clip and
        this Docker's box policy and clip convention, or whatever else ``model.convolve`` is -- and the plain one of the clash
        channel (Docker.py:32)."""
        from deeplocalproteindocking_amd.ops import VolumeConvolution
        model, emb = self.docking_model, self.embed_uncompiled_boxes
        convolve = getattr(model, "convolve", None) or VolumeConvolution(clip=getattr(model, "clip", 5.0), lib=self._lib)
        if isinstance(convolve, VolumeConvolution):
            convolve = VolumeConvolution(clip=convolve.clip, lib=self._lib, embed=emb, clip_mode=self.conventions.clip_mode)
        return convolve, VolumeConvolution(lib=self._lib, embed=emb)

    def _rotated_ligand(self, lig, ligand_forbidden=None, clash_provider=None):
        """``_search_unfused``'s ligand source for a search on volumes: the stored ligand volumes rotated by the stand-alone op;
        the forbidden volume re-projected by ``clash_provider(Rb)`` or the stored one rotated the same way (neither: no clash)."""
        dev, rotate = self.device, _PivotRotation(self)
        L = lig[0].shape[-1]
        lig_d = [v.to(dev) for v in lig]
        lf = None
        if ligand_forbidden is not None and clash_provider is None:
            lf = torch.as_tensor(ligand_forbidden, dtype=torch.float32).reshape(1, 1, L, L, L).to(dev)

        def ligand_batch(bid, Rb):
            nb = len(bid)
            forb = None
            if clash_provider is not None:
                forb = clash_provider(Rb).reshape(nb, 1, L, L, L).contiguous()
            elif lf is not None:
                forb = rotate(lf.expand(nb, -1, -1, -1, -1).contiguous(), Rb)
            return [rotate(v.unsqueeze(0).expand(nb, -1, -1, -1, -1).contiguous(), Rb) for v in lig_d], forb
        return ligand_batch

    def _search_unfused(self, path, rec, receptor_forbidden, ids, nbatch, ligand_batch, params):
        """The loop body of Docker.py:218-232 / :163-177 between the stand-alone HIP ops and the device top-K, ``nbatch``
        rotations at a time -> the list's entries.  ``ligand_batch(bid, Rb)`` -> the batch's ligand volumes and its forbidden
        volume ((nb, 1, L, L, L); None without clash).  Only the scoring goes by ``path``:
          ops   per-resolution correlation, then the HIP filter kernel (upsample + concat + MLP + mask multiply);
          call  ``V = self.docking_model(receptor_volumes, ligand_volumes)`` (Docker.py:229) really CALLED, whatever module
                that is -- the path of a user-defined filter / docking model -- then the mask multiply."""
        from deeplocalproteindocking_amd.ops import filter_volumes
        dev, model = self.device, self.docking_model
        L = rec[0].shape[-1]
        convolve, conv_noclip = self._convolutions()
        rec_d = [v.to(dev) for v in rec]
        rf = None
        if receptor_forbidden is not None:
            rf = torch.as_tensor(receptor_forbidden, dtype=torch.float32).reshape(1, 1, L, L, L).to(dev)
        top = DeviceTopList(self.max_conf, nbatch, dev, self._library(), exclusion=int(self.exclusion))
        top.set_restraints(self.restraint_table())
        top.reset()
        with torch.no_grad():
            for beg in range(0, len(ids), nbatch):
                bid = ids[beg:beg + nbatch]
                nb = len(bid)
                Rb = self.rot.R[bid].to(device=dev, dtype=torch.float32).contiguous()
                lig_b, forb = ligand_batch(bid, Rb)
                rec_b = [v.unsqueeze(0).expand(nb, -1, -1, -1, -1).contiguous() for v in rec_d]
                norm = None
                if rf is not None:
                    norm = conv_noclip(rf.expand(nb, -1, -1, -1, -1).contiguous(), forb).squeeze(1).contiguous()
                if path == "ops":
                    W1, b1, W2, b2 = params
                    V = filter_volumes([convolve(r, l) for r, l in zip(rec_b, lig_b)], W1, b1, W2, float(b2.reshape(-1)[0]),
                                       mask_norm=norm, threshold=model.threshold_clash, lib=self._lib)
                else:
                    V = model(rec_b, lig_b).reshape(nb, 2 * L, 2 * L, 2 * L).to(torch.float32)
                    if norm is not None:
                        V = torch.lt(norm, model.threshold_clash).to(dtype=torch.float32) * V
                    V = V.contiguous()
                bid_dev = torch.as_tensor(bid, dtype=torch.int32).to(dev)
                top.select(V.reshape(nb, -1), nb, None, bid_dev)
                top.merge(bid_dev, nb)
        return top.entries()

    def _gather(self, entries):
        """One all-gather of the fixed-size per-rank lists + deterministic merge (every rank)."""
        return all_gather_top_entries(entries, self.max_conf, self.world_size, self.process_group, self.device,
                                      always=self.collectives_with_one_rank)

    # ------------------------------------------------------------------ PDB-level entries
    def _need_backend(self):
        """The atom front end (TorchProteinLibrary's PDB2CoordsUnordered / Coords2TypedCoords /
        CoordsTranslate / CoordsRotate / TypedCoords2Volume, Docker.py:29-39): this build's
        ``CoordsBackend`` unless the constructor was given another one."""
        if self.coords_backend is None:
            from deeplocalproteindocking_amd.Utils.FullAtom import CoordsBackend
            self.coords_backend = CoordsBackend(lib=self._lib, splat=self.conventions.splat,
                                                atom_types=self.conventions.atom_types)
        return self.coords_backend

    def load_batch(self, filenames, bbox_center=True):
        """Docker.py:49-61 through the coords backend."""
        be = self._need_backend()
        coords, chains, resnames, resnums, atomnames, num_atoms = be.pdb2coords(filenames)
        coords, num_atoms_of_type, offsets = be.assign_types(coords, resnames, atomnames, num_atoms)
        num_atoms = getattr(be, "last_num_typed", num_atoms)        # untyped atoms (hydrogens) were dropped
        a, b = be.get_bbox(coords, num_atoms)
        if bbox_center:
            translation = -(a + b) * 0.5 + self.box_length / 2.0
        else:
            translation = -(a + b) * 0.5
        coords = be.translate(coords, translation, num_atoms)
        return coords, num_atoms_of_type, offsets, translation, num_atoms

    def prepare(self, ureceptor, uligand, group="SE3", slot=0, stream=None):
        """The rotation-independent part of ``dockSE3`` / ``dockE3`` for one target (Docker.py:184-209 / :135-161) ->
        ``PreparedPair``.  ``slot`` names the engine it fills (0 / 1), so that a sweep over targets (local_test.py:57-75)
        can prepare target n + 1 -- from a host thread of its own -- while target n is being searched in the other engine;
        its device work goes to the CALLER'S current stream, i.e. between two batches of the running search, never beside
        them.  No collective is issued here (the random receptor rotation is shared by ``dock*`` / the constructor, on the
        caller's thread).
        ``stream`` is a DIAGNOSTIC argument (scripts/prepare_race_probe.py) and warns: a preparation on a second stream puts the
        plugin's matrix-instruction convolution on the same CUs as the search's kernels, which on this hardware changes low
        mantissa bits of a few scores (inside the 1e-4 parity band, but the .dat is then not byte-reproducible; an OPEN
        defect, not root-caused: DESIGN.md section 8, EXPERIMENTS.md R5).  The product never passes it."""
        import contextlib
        import time
        import warnings
        if stream is not None:
            warnings.warn("dlpd: Docker.prepare(stream=...) runs the representation beside the search's kernels; on this hardware "
                          "that co-residency perturbs low bits of a few scores (results stay inside the 1e-4 parity band but are "
                          "not byte-reproducible) -- diagnostic use only", RuntimeWarning, stacklevel=2)
        t0 = time.perf_counter()
        if group not in ("SE3", "E3"):
            raise Exception("Unknown equivariance group", group)
        be = self._need_backend()
        model = self.docking_model
        model.eval()
        dev, L, res = self.device, self.box_size, self.resolution
        p = PreparedPair(group, ureceptor, uligand, slot)
        on_stream = stream is not None and dev.type == "cuda"
        with (torch.cuda.stream(stream) if on_stream else contextlib.nullcontext()), torch.no_grad():
            rcoords, rnat, roff, rT, rnatoms = self.load_batch([ureceptor], bbox_center=False)
            lcoords, lnat, loff, lT, lnatoms = self.load_batch([uligand], bbox_center=False)
            p.receptor_shift, p.ligand_shift = rT, lT
            if self.randomize_rot:
                rcoords = be.rotate(rcoords, self.randR, rnatoms)
            rcoords = be.translate(rcoords, self.box_center, rnatoms)
            p.receptor = be.project(rcoords, rnat, roff, L, res, dev)
            p.receptor_volumes = model.representation(p.receptor)
            p.receptor_forbidden = p.receptor.sum(dim=1)[0]
            p.ligand_atoms = be.to_device(lcoords, lnat, loff, dev)             # origin-centred ligand atoms
            if group == "SE3":
                lcoords_trans = be.translate(lcoords, self.box_center, lnatoms)
                ligand = be.project(lcoords_trans, lnat, loff, L, res, dev)
                p.ligand_volumes = model.representation(ligand)
            # the fused engine of a compiled box: receptor spectrum (+ ligand layouts) now, not at the start of the search
            rec = [v.reshape((-1,) + tuple(v.shape[-3:])) for v in p.receptor_volumes]
            params = fused_filter_parameters(model)
            if params is not None and rec[0].shape[-1] == L:
                eng = self._make_engine(rec, p.receptor_forbidden, self.launch_batch, params, slot=slot)
                if eng is not None and group == "SE3":
                    lig = [v.reshape((-1,) + tuple(v.shape[-3:])) for v in p.ligand_volumes]
                    # (the clash channel comes from re-projected atoms: the stored forbidden volume is never read)
                    eng.set_ligand(lig[0], torch.zeros(L, L, L), lig[1] if eng.C1 > 0 else None)
                p.engine = eng
                if eng is not None:
                    eng.holds_pair = p                   # (checked when the pair is docked: a later prepare() into the same
                                                         #  slot replaces the receptor / ligand this engine holds)
            if on_stream:
                p.ready = torch.cuda.Event()
                p.ready.record(stream)
        p.seconds = time.perf_counter() - t0
        return p

    def _prepared_for(self, prepared, ureceptor, uligand, group):
        if prepared is None:
            return self.prepare(ureceptor, uligand, group)
        if (prepared.group, prepared.ureceptor, prepared.uligand) != (group, ureceptor, uligand):
            raise Exception("Prepared pair does not belong to this call", prepared.group, prepared.ureceptor, prepared.uligand)
        if prepared.engine is not None and getattr(prepared.engine, "holds_pair", None) is not prepared:
            raise Exception("Prepared pair was overwritten: another pair was prepared into engine slot %d after it" % prepared.slot)
        prepared.wait(self.device)
        return prepared

    def dockSE3(self, ureceptor, uligand, batch_size, prepared=None):
        """Docker.py:184-238: representations computed once, ligand volumes rotated on the GPU, and
        the ligand forbidden volume re-projected from the rotated ATOMS every batch (Docker.py:221-224)
        -- by one kernel that rotates on the fly, without the reference's per-batch host round trip.
        ``batch_size`` (2 in local_test.py:71) only sizes the calls of a model that has to be called
        (generic path); the fused pipeline always launches ``self.launch_batch`` rotations.
        prepared: the ``PreparedPair`` of this target if ``prepare`` already ran (a sweep preparing targets ahead)."""
        be = self._need_backend()
        self.top_list = []
        self.docking_model.eval()
        self._share_random_rotation()
        p = self._prepared_for(prepared, ureceptor, uligand, "SE3")
        L, res, dev = self.box_size, self.resolution, self.device
        with torch.no_grad():
            lc, ln, lo = p.ligand_atoms

            def provider(Rb):   # rotate about the origin, translate to the box centre, project, sum types
                return be.project(lc, ln, lo, L, res, dev, R=Rb, shift=self.box_center, sum_types=True)

            self.dock_volumes(p.receptor_volumes, p.ligand_volumes, p.receptor_forbidden, None, batch_size=None,
                              clash_provider=provider, model_batch=batch_size, prepared=p)


    def dockE3(self, ureceptor, uligand, batch_size, prepared=None):
        """Docker.py:135-182: the ligand is rotated in coordinate space and re-projected and
        re-represented every batch (the plugin's cost), then scored by the same kernels: the fused
        engine takes the batch's volumes as they are (no volume rotation); the stand-alone ops, or a
        call of the model itself, where the engine has no layout for the model (``_search_plan``).
        The two halves of a batch run one after the other on the caller's stream (``_dockE3_fused``).
        ``batch_size`` only sizes the calls of a model that has to be called, as in ``dockSE3``."""
        be = self._need_backend()
        self.top_list = []
        model = self.docking_model
        model.eval()
        dev, L = self.device, self.box_size
        self._share_random_rotation()
        p = self._prepared_for(prepared, ureceptor, uligand, "E3")
        ids = self.shard(self.rot.R.shape[0])
        with torch.no_grad():
            lc, ln, lo = p.ligand_atoms
            rec = [v.reshape((-1,) + tuple(v.shape[-3:])) for v in p.receptor_volumes]
            params = fused_filter_parameters(model)
            path, eng, Lc = self._search_plan(rec, p.receptor_forbidden, params, self.launch_batch, p.engine)

            def represent(bid):
                """rotate + translate + project in one kernel (Docker.py:163-165), then the plugin (Docker.py:166-167)"""
                Rb = self.rot.R[bid].to(device=dev, dtype=torch.float32).contiguous()
                # (_project_cells: set by _dockE3_fused when the plugin and the engine go by occupancy maps -- the projection
                #  then writes only the cells the atoms reach)
                ligand = be.project(lc, ln, lo, L, self.resolution, dev, R=Rb, shift=self.box_center,
                                    cells=bool(getattr(self, "_project_cells", False)))
                # the forbidden volume = the sum over the atom types (Docker.py:169): projected once more with the types summed in
                # the accumulator (33 MB) instead of a pass over the eleven volumes -- the integer sum of the types' fixed-point
                # densities converted once: equal to it bit for bit while every type stays below 4 per voxel (accumulator < 2^24,
                # each type's own float conversion is exact); above that the two differ by float32 rounding of either.  Only the
                # fused loop takes it; the unfused one sums the volumes as the reference does
                ligand.dlpd_type_sum = be.project(lc, ln, lo, L, self.resolution, dev, R=Rb, shift=self.box_center, sum_types=True)[:, 0]
                return ligand, model.representation(ligand)

            if eng is not None:
                nbatch = self.launch_batch
                eng.reset_top()
                self._dockE3_fused(eng, [ids[beg:beg + nbatch] for beg in range(0, len(ids), nbatch)], represent, Lc, nbatch)
                entries = eng.top_entries()
            else:
                def ligand_batch(bid, Rb):
                    ligand, ligand_volumes = represent(bid)
                    return ligand_volumes, ligand.sum(dim=1, keepdim=True)
                entries = self._search_unfused(path, rec, p.receptor_forbidden, ids,
                                               self.launch_batch if path == "ops" else int(batch_size), ligand_batch, params)
        self.top_list = DeviceTopList.to_top_list(self._gather(entries), 2 * L)
        self.write_conformations()

    def _dockE3_fused(self, eng, batches, represent, Lc, nbatch):
        """The batch loop of dockE3 on the fused engine: projection + representation of a batch, then the engine's half,
        on ONE stream.  (Round 5 built the plugin's half of batch i + 1 on a second stream beside the engine's half of
        batch i: no gain -- 15.08 against 15.03 ms per launch, both halves fill the chip -- and that co-residency of the
        plugin's matrix-instruction convolution with the pipeline's LDS kernels is exactly what perturbs the pipeline's low
        bits on this hardware, EXPERIMENTS.md R5; removed.)"""
        dev = self.device
        ebuf = {}

        def volumes_of(ligand, ligand_volumes, nb, slot):
            forb = getattr(ligand, "dlpd_type_sum", None)
            vols = (ligand_volumes[0], forb if forb is not None else ligand.sum(dim=1), ligand_volumes[1] if eng.C1 else None)
            if Lc:
                # the batch's volumes into the corner of buffers that were zeroed ONCE (not three allocations and zero
                # fills per batch); two sets when the plugin runs ahead of the engine
                if slot not in ebuf:
                    ebuf[slot] = [torch.zeros((nbatch,) + tuple(v.shape[1:-3]) + (le, le, le), dtype=torch.float32, device=dev)
                                  if v is not None else None for v, le in zip(vols, (Lc, Lc, Lc // 2))]
                for buf, v in zip(ebuf[slot], vols):
                    if v is not None:
                        buf[:nb][..., :v.shape[-3], :v.shape[-2], :v.shape[-1]] = v
                vols = tuple(None if buf is None else buf[:nb] for buf in ebuf[slot])
            return vols

        # A plugin whose layers carry occupancy maps (E3MultiResRepr4x4: bias-free convolutions) hands the maps on with its
        # volumes; the engine's K1 then never reads an empty cell, so the plugin need not WRITE the tiles it skips
        # (``outputs_with_maps``).  Not with an embedded box: the copy into the larger box reads every voxel.
        import contextlib
        rep = getattr(self.docking_model, "representation", None)
        # (clip_mode "input" clamps every voxel of the batch's volumes: maps are not combined with it)
        maps_ok = (not Lc) and eng._in_clip is None
        with_maps = maps_ok and bool(getattr(rep, "supports_unwritten_outputs", False)) and self.unwritten_activations
        from deeplocalproteindocking_amd import ops as _ops
        cells_ok = with_maps and bool(getattr(rep, "use_tile_occupancy", False)) and bool(getattr(rep, "use_hip_conv", False)) and \
            _ops.CONV_PRECISION == "split_bf16" and self.device.type == "cuda"
        for bid in batches:
            self._project_cells = cells_ok
            try:
                with (rep.outputs_with_maps() if with_maps else contextlib.nullcontext()):
                    ligand, ligand_volumes = represent(bid)
            finally:
                self._project_cells = False
            bid_dev = torch.as_tensor(bid, dtype=torch.int32).to(dev)
            occ = None
            if maps_ok:
                o0 = getattr(ligand_volumes[0], "dlpd_occupancy", None)
                o1 = getattr(ligand_volumes[1], "dlpd_occupancy", None) if eng.C1 else None
                occ = (o0, o1) if (o0 is not None or o1 is not None) else None
            eng.step(None, bid_dev, volumes=volumes_of(ligand, ligand_volumes, len(bid), 0), occupancy=occ)
