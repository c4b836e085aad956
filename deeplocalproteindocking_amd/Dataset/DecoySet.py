"""Training sets from this build's own searches, in the layout the reference's training stream reads
(scripts/Dataset/make_dataset_split.py:36-46 writes it there, src/Dataset/SplitComplexDataset.py:41-68 reads it):

    <dataset_dir>/Description/<subset>            one target name per line
    <dataset_dir>/Description/<target>.dat        header ``receptor ligand lrmsd irmsd fnat fnonnat quality``, one decoy per row
    <dataset_dir>/<decoys_dirname>/...            the receptor file (once per target) and one posed ligand file per decoy

The reference made its decoys with HEX, NOLB and ProFit; here they are poses -- the list a search ends with and poses round the
native one (``near_native_poses``, the part NOLB's near-native set plays there) -- labelled by ``Docker.evaluate(fnonnat=True)``.
BUILD-DEFINED: the reference has no counterpart of these functions, only of the files they write."""
import os

import numpy as np

from deeplocalproteindocking_amd.Results import InterfaceSelection as isel

HEADER = "receptor\tligand\tlrmsd\tirmsd\tfnat\tfnonnat\tquality\n"
ROW = "%s\t%s\t%f\t%f\t%f\t%f\t%d\n"


def native_pose(native):
    """(R (3, 3), t (3)) float64, t in Angstrom: the pose that carries the unbound ligand (about its bounding-box centre) onto
    the bound one in the docking frame -- the Kabsch fit of ``native.ligand_ca`` onto ``native.target_ca``."""
    R, t = isel.kabsch_fit(np.asarray(native.ligand_ca, dtype=np.float64), np.asarray(native.target_ca, dtype=np.float64))
    return R, t


def _rotation(omega):
    """Rodrigues: the rotation by |omega| radians about omega"""
    angle = float(np.linalg.norm(omega))
    if angle == 0.0:
        return np.eye(3)
    k = omega / angle
    Kx = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(angle) * Kx + (1.0 - np.cos(angle)) * (Kx @ Kx)


def near_native_poses(native, n, angle=5.0, shift=2.0, seed=0):
    """(n, 12) float64 poses in the frame of a .dat file (R row-major, then t in Angstrom) round the native one: the first is
    the native pose itself, the others turn it by a rotation vector N(0, ``angle`` degrees) per component about the ligand's
    interface centre (where the native pose puts the ligand's interface C-alphas) and shift it by N(0, ``shift`` Angstrom) per
    component.  Seeded: equal arguments give equal poses."""
    rs = np.random.RandomState(int(seed))
    Rn, tn = native_pose(native)
    y = np.concatenate([np.asarray(p[1], dtype=np.float64).reshape(-1, 3) for p in native.pairs])
    centre = (y @ Rn.T + tn).mean(axis=0)
    out = np.zeros((int(n), 12))
    for k in range(int(n)):
        if k == 0:
            R, t = Rn, tn
        else:
            Q = _rotation(rs.normal(size=3) * np.radians(angle))
            R, t = Q @ Rn, Q @ (tn - centre) + centre + rs.normal(size=3) * shift
        out[k, :9], out[k, 9:] = R.reshape(-1), t
    return out


def pose_entries(poses, docker):
    """(K, 12) poses in the frame of a .dat file -> ``refined_list`` entries of ``docker`` (R, t in voxels, score 0.0, index):
    the inverse of ``Docker.dat_frame_poses``, its ``randomize_rot`` included, so that ``docker.evaluate(native, entries)``
    measures these poses"""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 12)
    Q = docker.randR.squeeze().double().numpy() if docker.randomize_rot else np.eye(3)
    return [(Q @ p[:9].reshape(3, 3), tuple(float(v) for v in (Q @ p[9:]) / float(docker.resolution)), 0.0, k) for k, p in enumerate(poses)]


def posed_ligand_lines(lines, R, t, c_lig, c_rec):
    """The ATOM lines of a ligand file with columns 31-54 replaced by x' = R (x - c_lig) + t + c_rec (``%8.3f``): the ligand
    where the pose puts it, next to the receptor file as it stands"""
    out = []
    for line in lines:
        if not line.startswith("ATOM"):
            continue
        x = np.array([float(line[30:38]), float(line[38:46]), float(line[46:54])])
        p = R @ (x - c_lig) + t + c_rec
        out.append(line[:30] + "%8.3f%8.3f%8.3f" % tuple(p) + line[54:].rstrip("\n") + "\n")
    return out


def write_decoy_set(dataset_dir, target, receptor_pdb, ligand_pdb, poses, evaluation, decoys_dirname="Decoys", subset="training_set.dat",
                    description_dir="Description"):
    """One target of a training set.  ``poses``: (K, 12) float64 in the frame of a .dat file (``Docker.dat_frame_poses``: R
    row-major, then t in Angstrom); ``evaluation``: ``Docker.evaluate(native, poses, fnonnat=True)`` of the same poses.
    Writes <dataset_dir>/<decoys_dirname>/<target>_r.pdb (the receptor's ATOM lines, once), <target>_l_<k>.pdb (the posed
    ligand of decoy k), <dataset_dir>/<description_dir>/<target>.dat and appends the target to the subset file unless it is
    named there.  The table names the files by their full paths; a reader that re-roots them (the last two components under its
    own dataset_dir, SplitComplexDataset.py:62-65) finds them wherever the set is moved.  -> the path of the table."""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 12)
    K = poses.shape[0]
    for key in ("lrmsd", "irmsd", "fnat", "fnonnat", "capri"):
        if key not in evaluation or len(evaluation[key]) != K:
            raise RuntimeError("dlpd: write_decoy_set needs Docker.evaluate(fnonnat=True) of the same %d poses (%s)" % (K, key))
    if os.sep in decoys_dirname or not decoys_dirname:
        raise RuntimeError("dlpd: decoys_dirname is one directory name under dataset_dir")
    ddir, desc = os.path.join(dataset_dir, decoys_dirname), os.path.join(dataset_dir, description_dir)
    os.makedirs(ddir, exist_ok=True)
    os.makedirs(desc, exist_ok=True)
    c_rec, c_lig = isel.bbox_centre(isel.read_structure(receptor_pdb)), isel.bbox_centre(isel.read_structure(ligand_pdb))
    rec_name = os.path.join(ddir, "%s_r.pdb" % target)
    with open(receptor_pdb) as fin, open(rec_name, "w") as fout:
        fout.writelines(ln.rstrip("\n") + "\n" for ln in fin if ln.startswith("ATOM"))
    with open(ligand_pdb) as fin:
        lig_lines = fin.readlines()
    rows = []
    for k in range(K):
        lig_name = os.path.join(ddir, "%s_l_%d.pdb" % (target, k))
        with open(lig_name, "w") as fout:
            fout.writelines(posed_ligand_lines(lig_lines, poses[k, :9].reshape(3, 3), poses[k, 9:], c_lig, c_rec))
        rows.append(ROW % (rec_name, lig_name, evaluation["lrmsd"][k], evaluation["irmsd"][k], evaluation["fnat"][k],
                           evaluation["fnonnat"][k], int(evaluation["capri"][k])))
    table = os.path.join(desc, "%s.dat" % target)
    with open(table, "w") as fout:
        fout.write(HEADER)
        fout.writelines(rows)
    subset_path = os.path.join(desc, subset)
    named = []
    if os.path.exists(subset_path):
        with open(subset_path) as fin:
            named = [ln.split()[0] for ln in fin if ln.split()]
    if target not in named:
        with open(subset_path, "a") as fout:
            fout.write("%s\n" % target)
    return table
