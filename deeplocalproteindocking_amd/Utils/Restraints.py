"""Distance restraints of a search (include/dlpd.h dlpd_topk_restrain; build-defined, host side, numpy float64).

A restraint says that a point of the ligand lies within [dmin, dmax] Angstrom of a point of the receptor in the docked complex.
Poses follow ``Docker.cluster`` / ``Docker.evaluate``: list entry (rot, x, y, z) carries the ligand point a (Angstrom, ligand
centred on the origin as ``PreparedPair.ligand_atoms`` holds it) to R_rot a + resolution t, t = ``Docker.signed_translation``;
the receptor point b is in Angstrom in the search frame (origin-centred, after randR).  The kernels and ``allowed`` evaluate
the predicate in integers, in units of 1/256 voxel -- 0.005 A at 1.25 A resolution, the step of the test."""
import numpy as np

MAX_RESTRAINTS = 32
UNIT = 256                     # integer units per voxel
MAX_CENTRE = 1 << 20           # |c|, integer units
MAX_HI = 1 << 21               # hi, integer units


class Restraint(object):
    """dmin <= |pose(ligand_point) - receptor_point| <= dmax, both points (3,) in Angstrom in the frames named above."""

    def __init__(self, receptor_point, ligand_point, dmax, dmin=0.0):
        self.receptor_point = np.asarray(receptor_point, dtype=np.float64).reshape(3)
        self.ligand_point = np.asarray(ligand_point, dtype=np.float64).reshape(3)
        self.dmax, self.dmin = float(dmax), float(dmin)
        if not (np.isfinite(self.receptor_point).all() and np.isfinite(self.ligand_point).all()):
            raise ValueError("restraint: a point is not finite")
        if not (0.0 <= self.dmin <= self.dmax < np.inf):
            raise ValueError("restraint: needs 0 <= dmin <= dmax < inf, got dmin %r, dmax %r" % (dmin, dmax))

    def __repr__(self):
        return "Restraint(%s, %s, dmax=%g, dmin=%g)" % (self.receptor_point.tolist(), self.ligand_point.tolist(), self.dmax, self.dmin)


class RestraintTable(object):
    """What the kernels read: centres int32 (nrot, J, 3), bounds int64 (2 J,) -- lo^2 of the J restraints, then hi^2 -- and
    need.  ``lo`` / ``hi`` int64 (J,) are the unsquared bounds."""

    def __init__(self, centres, lo, hi, need):
        self.centres = np.ascontiguousarray(centres, dtype=np.int32)
        self.lo, self.hi = np.asarray(lo, dtype=np.int64), np.asarray(hi, dtype=np.int64)
        self.bounds = np.ascontiguousarray(np.concatenate([self.lo * self.lo, self.hi * self.hi]), dtype=np.int64)
        self.J, self.need = int(self.centres.shape[1]), int(need)

    @property
    def nrot(self):
        return int(self.centres.shape[0])

    def cube_volume(self):
        """Voxels in the bounding cubes of the J balls before clipping to a grid (the same for every rotation): what a rebuild
        of a candidate list walks at most."""
        side = 2 * ((self.hi + UNIT - 1) // UNIT) + 1
        return int((side ** 3).sum())


def restraint_table(R_all, restraints, resolution, need=None):
    """R_all (nrot, 3, 3), restraints: 1..32 ``Restraint`` -> ``RestraintTable`` for every rotation of the set.  need: how many
    of them a pose must satisfy (None: all).  Float64 throughout; centres round half to even, as numpy's rint does."""
    restraints = list(restraints)
    J = len(restraints)
    if not 1 <= J <= MAX_RESTRAINTS:
        raise ValueError("restraints: 1..%d per set, got %d" % (MAX_RESTRAINTS, J))
    need = J if need is None else int(need)
    if not 1 <= need <= J:
        raise ValueError("restraints: restraints_needed %d outside 1..%d" % (need, J))
    R = np.asarray(R_all.detach().cpu().numpy() if hasattr(R_all, "detach") else R_all, dtype=np.float64).reshape(-1, 3, 3)
    res = float(resolution)
    a = np.stack([r.ligand_point for r in restraints])                  # (J, 3)
    b = np.stack([r.receptor_point for r in restraints])
    c = np.rint(UNIT * (b[None] - np.einsum("rij,kj->rki", R, a)) / res)
    if not (np.abs(c) <= MAX_CENTRE).all():
        raise ValueError("restraints: a centre lies more than %d voxels from the origin" % (MAX_CENTRE // UNIT))
    lo = np.rint(UNIT * np.array([r.dmin for r in restraints]) / res)
    hi = np.rint(UNIT * np.array([r.dmax for r in restraints]) / res)
    if not (hi <= MAX_HI).all():
        raise ValueError("restraints: dmax above %g voxels" % (MAX_HI / UNIT))
    return RestraintTable(c.astype(np.int32), lo.astype(np.int64), hi.astype(np.int64), need)


def satisfied(table, rot, t_signed):
    """Number of restraints each signed translation satisfies.  rot: one rotation index or an array like t_signed's leading
    shape; t_signed (..., 3) in voxels -- integers for list entries; fractions (a ``refined_list``) are taken as they stand,
    in float64, against the same integer centres and bounds."""
    t = np.asarray(t_signed)
    c = table.centres[np.asarray(rot, dtype=np.int64)].astype(np.int64)          # (..., J, 3)
    lo2, hi2 = table.bounds[:table.J], table.bounds[table.J:]
    if np.issubdtype(t.dtype, np.integer):
        d = UNIT * t.astype(np.int64)[..., None, :] - c
        d2 = (d * d).sum(axis=-1)
    else:
        d = UNIT * t.astype(np.float64)[..., None, :] - c
        d2 = (d * d).sum(axis=-1)
    return ((d2 >= lo2) & (d2 <= hi2)).sum(axis=-1)


def allowed(table, rot, t_signed):
    """The definition: at least ``table.need`` restraints satisfied."""
    return satisfied(table, rot, t_signed) >= table.need


def select_point(pdb_file, selection):
    """"CHAIN:RESNUM[:ATOM]" -> (3,) float64 in the file's own frame.  ATOM defaults to CA; ``*`` is the centroid of the residue's
    heavy atoms; ``_`` names a blank chain."""
    from .FullAtom import read_pdb_atoms
    parts = str(selection).split(":")
    if len(parts) not in (2, 3) or not parts[0] or not parts[1]:
        raise ValueError("selection %r in %s: expected CHAIN:RESNUM[:ATOM]" % (selection, pdb_file))
    chain = " " if parts[0] == "_" else parts[0]
    try:
        resnum = int(parts[1])
    except ValueError:
        raise ValueError("selection %r in %s: residue number %r is not an integer" % (selection, pdb_file, parts[1]))
    atom = parts[2] if len(parts) == 3 and parts[2] else "CA"
    xyz, chains, _, resnums, atomnames = read_pdb_atoms(pdb_file)
    res = np.array([c == chain and int(n) == resnum for c, n in zip(chains, resnums)], dtype=bool)
    if not res.any():
        raise ValueError("selection %r: no residue %d in chain %r of %s" % (selection, resnum, parts[0], pdb_file))
    if atom == "*":
        return xyz[res].mean(axis=0)
    hit = res & np.array([a == atom for a in atomnames], dtype=bool)
    if not hit.any():
        raise ValueError("selection %r: residue %d of chain %r in %s has no atom %r" % (selection, resnum, parts[0], pdb_file, atom))
    return xyz[np.nonzero(hit)[0][0]].copy()
