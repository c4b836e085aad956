"""Interface selection for the I-RMSD evaluation of a ``.dat`` file: what
/root/reference/scripts/Results/Benchmark/EvaluateBenchmark.py:44-113 does between ``parse_output`` and the RMSD
loop, with the pieces of DockingBenchmark.py / VisualizeBenchmark.py it calls:

  get_contacts (DockingBenchmark.py:291-327)        residues of the BOUND receptor / ligand with an atom pair closer than
                                                    ``contact_dist`` (5 A); standard amino acids only, residues with an
                                                    insertion code skipped -> lists of (chain, resnum, one-letter name)
  get_chain_seq (:23-36)                            per-chain sequence + residue numbers (same filters)
  get_best_match (:88-121) + get_alignment          bound chain -> unbound chain + residue alignment
      (scripts/Dataset/global_alignment.py:35-70)
  transfer_selection (:397-420)                     bound selection -> unbound selection through that alignment;
                                                    unaligned residues are dropped from BOTH, a residue-name mismatch
                                                    raises "Residues are not matching"
  select_CA / select_residues_list                  C-alpha coordinates of a selection, in the selection's order
      (VisualizeBenchmark.py:53-86)
  get_irmsd loop (EvaluateBenchmark.py:60-113)      per conformation the minimum superposed RMSD over interface pairs

Build-defined where the reference leans on absent packages (parity unpinned, no vectors in the reference tree):
BioPython's ``pairwise2.align.globaldx`` with BLOSUM62 is replaced by a Needleman-Wunsch global alignment with identity
scoring and free gaps (the bound / unbound chains of a benchmark entry are the same protein: both give the identity
mapping with gaps at missing residues); chains are paired by sequence identity first, C-alpha distance second; the
symmetric re-labellings of homo-oligomers (``get_symmetric_selections``, needs the external AnAnaS tool) are not
enumerated -- one assembly per target."""
from collections import OrderedDict

import numpy as np
import torch

THREE_TO_ONE = {"ALA": "A", "CYS": "C", "ASP": "D", "GLU": "E", "PHE": "F", "GLY": "G", "HIS": "H", "ILE": "I", "LYS": "K",
                "LEU": "L", "MET": "M", "ASN": "N", "PRO": "P", "GLN": "Q", "ARG": "R", "SER": "S", "THR": "T", "VAL": "V",
                "TRP": "W", "TYR": "Y"}


def read_structure(filename):
    """ATOM records of the first model -> dict of arrays: xyz (n,3) f64, chain, resnum, icode, resname, atomname
    (alternate locations other than ' ' / 'A' dropped, as the docking front end does)."""
    xyz, chain, resnum, icode, resname, atomname = [], [], [], [], [], []
    with open(filename) as fin:
        for line in fin:
            if line.startswith("ENDMDL"):
                break
            if not line.startswith("ATOM") or line[16] not in (" ", "A"):
                continue
            atomname.append(line[12:16].strip())
            resname.append(line[17:20].strip())
            chain.append(line[21])
            resnum.append(int(line[22:26]))
            icode.append(line[26])
            xyz.append((float(line[30:38]), float(line[38:46]), float(line[46:54])))
    return {"path": filename, "xyz": np.asarray(xyz, dtype=np.float64).reshape(-1, 3), "chain": np.asarray(chain),
            "resnum": np.asarray(resnum, dtype=np.int64), "icode": np.asarray(icode), "resname": np.asarray(resname),
            "atomname": np.asarray(atomname)}


def _standard(s):
    return np.array([(r in THREE_TO_ONE) and (i == " ") for r, i in zip(s["resname"], s["icode"])], dtype=bool)


def chain_sequences(s):
    """chain -> (one-letter sequence, residue numbers): DockingBenchmark.get_chain_seq per chain, file order."""
    out = OrderedDict()
    ok = _standard(s)
    for i in np.nonzero(ok)[0]:
        c, n = str(s["chain"][i]), int(s["resnum"][i])
        seq, nums = out.setdefault(c, ([], []))
        if not nums or nums[-1] != n:
            seq.append(THREE_TO_ONE[str(s["resname"][i])])
            nums.append(n)
    return OrderedDict((c, ("".join(v[0]), v[1])) for c, v in out.items())


def align_global(seq1, seq2):
    """Global alignment with identity scoring (+1 match, 0 mismatch) and free gaps -- the longest common subsequence --
    -> (pairs [(i, j)] of aligned IDENTICAL positions, identity = matches / alignment columns).  Stand-in for
    global_alignment.get_alignment (BioPython absent); residues that differ between the two chains come out unaligned and
    are dropped from a transferred selection, where the reference would raise "Residues are not matching"."""
    n, m = len(seq1), len(seq2)
    a = np.frombuffer(seq1.encode(), dtype=np.uint8)
    b = np.frombuffer(seq2.encode(), dtype=np.uint8)
    S = np.zeros((n + 1, m + 1), dtype=np.int32)
    for i in range(1, n + 1):
        S[i, 1:] = np.maximum.accumulate(np.maximum(S[i - 1, :-1] + (a[i - 1] == b), S[i - 1, 1:]))
    pairs, i, j = [], n, m
    while i > 0 and j > 0:
        if a[i - 1] == b[j - 1] and S[i, j] == S[i - 1, j - 1] + 1:
            pairs.append((i - 1, j - 1))
            i, j = i - 1, j - 1
        elif S[i, j] == S[i - 1, j]:
            i -= 1
        else:
            j -= 1
    pairs.reverse()
    cols = n + m - len(pairs)                  # every unmatched residue of either chain is a column of its own
    return pairs, (len(pairs) / float(cols) if cols else 0.0)


def _ca_of(s, chain, resnum):
    sel = np.nonzero((s["chain"] == chain) & (s["resnum"] == resnum) & (s["atomname"] == "CA") & (s["icode"] == " "))[0]
    return s["xyz"][sel[0]] if len(sel) else None


def best_chain_match(s1, s2, min_identity=0.9):
    """chain of s1 -> (chain of s2, identity, {residue index in s1's chain: residue index in s2's chain}):
    DockingBenchmark.get_best_match -- the partner is the chain with the highest identity (ties: the smaller mean C-alpha
    distance over the aligned residues, the reference's criterion); below ``min_identity`` the match is rejected like
    the reference's "Alignment is bad"."""
    c1, c2 = chain_sequences(s1), chain_sequences(s2)
    match = {}
    for ch1, (seq1, nums1) in c1.items():
        best = None
        for ch2, (seq2, nums2) in c2.items():
            if not seq1 or not seq2:
                raise Exception("Chain is empty")
            pairs, ident = align_global(seq1, seq2)
            d, k = 0.0, 0
            for i, j in pairs:
                p, q = _ca_of(s1, ch1, nums1[i]), _ca_of(s2, ch2, nums2[j])
                if p is not None and q is not None:
                    d, k = d + float(np.linalg.norm(p - q)), k + 1
            key = (-ident, d / max(k, 1))
            if best is None or key < best[0]:
                best = (key, ch2, ident, dict(pairs))
        if best[2] < min_identity:
            raise Exception("Alignment is bad", ch1, best[1], best[2])
        match[ch1] = (best[1], best[2], best[3])
    return match


def get_contacts(receptor, ligand, contact_dist=5.0):
    """Residues of the (bound) receptor / ligand with any atom pair within ``contact_dist`` ->
    (receptor selection, ligand selection), each a sorted list of (chain, resnum, one-letter name)."""
    from scipy.spatial import cKDTree
    ok_r, ok_l = _standard(receptor), _standard(ligand)
    ir, il = np.nonzero(ok_r)[0], np.nonzero(ok_l)[0]
    pairs = cKDTree(ligand["xyz"][il]).query_ball_tree(cKDTree(receptor["xyz"][ir]), contact_dist)
    rec_sel, lig_sel = set(), set()
    for a, hits in enumerate(pairs):
        if not hits:
            continue
        i = il[a]
        lig_sel.add((str(ligand["chain"][i]), int(ligand["resnum"][i]), THREE_TO_ONE[str(ligand["resname"][i])]))
        for h in hits:
            j = ir[h]
            rec_sel.add((str(receptor["chain"][j]), int(receptor["resnum"][j]), THREE_TO_ONE[str(receptor["resname"][j])]))
    return sorted(rec_sel), sorted(lig_sel)


def transfer_selection(selection_src, src, dst, match):
    """DockingBenchmark.transfer_selection: the residues of ``selection_src`` (on ``src``) as residues of ``dst``;
    returns (kept source selection, destination selection), aligned entry by entry."""
    seq_src, seq_dst = chain_sequences(src), chain_sequences(dst)
    kept, out = [], []
    for chain_id, res_num, res in selection_src:
        matching_chain, _, alignment = match[chain_id]
        res_idx = seq_src[chain_id][1].index(res_num)
        if res_idx not in alignment:
            continue                                             # removed from the source selection too
        k = alignment[res_idx]
        matching_res_num, matching_res = seq_dst[matching_chain][1][k], seq_dst[matching_chain][0][k]
        if matching_res != res:
            raise Exception("Residues are not matching", chain_id, res_num, res, ":", matching_chain, matching_res_num,
                            matching_res)
        kept.append((chain_id, res_num, res))
        out.append((matching_chain, matching_res_num, matching_res))
    return kept, out


def select_ca(s, selection, shift=None):
    """C-alpha coordinates (n,3) float64 tensor of the selected residues in the selection's order (select_CA followed by
    select_residues_list); residues without a C-alpha are an error -- the two sides of an RMSD must stay aligned."""
    rows = []
    for chain, resnum, _ in selection:
        p = _ca_of(s, chain, resnum)
        if p is None:
            raise Exception("Residue has no CA atom", chain, resnum)
        rows.append(p)
    xyz = torch.from_numpy(np.asarray(rows, dtype=np.float64).reshape(-1, 3))
    return xyz if shift is None else xyz + torch.as_tensor(shift, dtype=torch.double).reshape(1, 3)


def bbox_centre(s):
    """centre of the bounding box of ALL atoms (DockerParser.load_protein's frame, DockerParser.py:70-74)"""
    return 0.5 * (s["xyz"].min(axis=0) + s["xyz"].max(axis=0))


def unbound_interfaces(bound_receptor, bound_ligand, unbound_receptor, unbound_ligand, contact_dist=5.0):
    """DockingBenchmark.get_unbound_interfaces for one assembly: [(urec_sel, ulig_sel, brec_sel, blig_sel)] with the
    four selections aligned entry by entry (receptor with receptor, ligand with ligand)."""
    brec_cont, blig_cont = get_contacts(bound_receptor, bound_ligand, contact_dist)
    rec_match = best_chain_match(bound_receptor, unbound_receptor)
    lig_match = best_chain_match(bound_ligand, unbound_ligand)
    brec_sel, urec_sel = transfer_selection(brec_cont, bound_receptor, unbound_receptor, rec_match)
    blig_sel, ulig_sel = transfer_selection(blig_cont, bound_ligand, unbound_ligand, lig_match)
    return [(urec_sel, ulig_sel, brec_sel, blig_sel)]


def evaluate_target(parser, target_name, bound_receptor_pdb, bound_ligand_pdb, unbound_receptor_pdb, unbound_ligand_pdb,
                    num_conf=None, contact_dist=5.0):
    """EvaluateBenchmark.get_irmsd for one target: the interface RMSD of every conformation of
    ``<decoys_dir>/<target_name>.dat`` (None if the file is missing).  The unbound structures are taken in the docking
    frame -- each centred on its own bounding-box centre, the ligand then placed by the pose."""
    if parser.parse_output(target_name, header_only=False) is None:
        return None
    br, bl = read_structure(bound_receptor_pdb), read_structure(bound_ligand_pdb)
    ur, ul = read_structure(unbound_receptor_pdb), read_structure(unbound_ligand_pdb)
    mobile, static = [], []
    for urec_sel, ulig_sel, brec_sel, blig_sel in unbound_interfaces(br, bl, ur, ul, contact_dist):
        mobile.append((select_ca(ur, urec_sel, -bbox_centre(ur)), select_ca(ul, ulig_sel, -bbox_centre(ul))))
        static.append(torch.cat([select_ca(br, brec_sel), select_ca(bl, blig_sel)], dim=0))
    n = len(parser.target_dict["conformations"])
    n = n if num_conf is None else min(n, int(num_conf))
    return [parser.interface_rmsd(mobile, static, i) for i in range(n)]


# ----------------------------------------------------------------------------------------------------------------------
# Evaluation on the device (csrc/dlpd_evaluate.h): I-RMSD, L-RMSD, fraction of native contacts, CAPRI class
# ----------------------------------------------------------------------------------------------------------------------

def _residue(s, i):
    return (str(s["chain"][i]), int(s["resnum"][i]), THREE_TO_ONE[str(s["resname"][i])])


def native_contact_pairs(receptor, ligand, contact_dist=5.0):
    """The native contacts of a (bound) complex: the residue pairs with any atom pair within ``contact_dist`` -- the
    ``contacts`` set of processing_utils.py:183-216 -- under the filters of ``get_contacts`` (standard amino acids, no
    insertion code) -> sorted list of ((chain, resnum, name) of the receptor, (chain, resnum, name) of the ligand)."""
    from scipy.spatial import cKDTree
    ir, il = np.nonzero(_standard(receptor))[0], np.nonzero(_standard(ligand))[0]
    if not len(ir) or not len(il):
        return []
    hits = cKDTree(ligand["xyz"][il]).query_ball_tree(cKDTree(receptor["xyz"][ir]), contact_dist)
    pairs = set()
    for a, hs in enumerate(hits):
        for h in hs:
            pairs.add((_residue(receptor, ir[h]), _residue(ligand, il[a])))
    return sorted(pairs)


def transfer_pairs(pairs, bound_receptor, unbound_receptor, receptor_match, bound_ligand, unbound_ligand, ligand_match):
    """Residue pairs of the bound complex as residue pairs of the unbound structures, each residue through
    ``transfer_selection``; a pair with an unaligned residue is dropped -> (kept bound pairs, unbound pairs), entry by entry."""
    def table(residues, src, dst, match):
        out = {}
        for res in sorted(set(residues)):
            kept, moved = transfer_selection([res], src, dst, match)
            out[res] = moved[0] if kept else None
        return out
    rec = table([p[0] for p in pairs], bound_receptor, unbound_receptor, receptor_match)
    lig = table([p[1] for p in pairs], bound_ligand, unbound_ligand, ligand_match)
    kept = [p for p in pairs if rec[p[0]] is not None and lig[p[1]] is not None]
    return kept, [(rec[p[0]], lig[p[1]]) for p in kept]


def aligned_ca(bound, unbound, match):
    """C-alpha coordinates of every aligned residue pair that has one in both structures -> (bound (m, 3), unbound (m, 3))"""
    sb, su = chain_sequences(bound), chain_sequences(unbound)
    pb, pu = [], []
    for ch, (other, _, alignment) in match.items():
        for i in sorted(alignment):
            p, q = _ca_of(bound, ch, sb[ch][1][i]), _ca_of(unbound, other, su[other][1][alignment[i]])
            if p is not None and q is not None:
                pb.append(p)
                pu.append(q)
    return np.asarray(pb, dtype=np.float64).reshape(-1, 3), np.asarray(pu, dtype=np.float64).reshape(-1, 3)


def kabsch_fit(mobile, static):
    """The rigid motion x -> Q x + s that carries ``mobile`` (n, 3) onto ``static`` (n, 3) with the least RMSD (float64 SVD)"""
    cm, cs = mobile.mean(axis=0), static.mean(axis=0)
    U, _, Vt = np.linalg.svd((mobile - cm).T @ (static - cs))
    d = np.sign(np.linalg.det(Vt.T @ U.T))
    Q = Vt.T @ np.diag([1.0, 1.0, d if d != 0 else 1.0]) @ U.T
    return Q, cs - Q @ cm


def _residue_atoms(s, residue, shift):
    sel = (s["chain"] == residue[0]) & (s["resnum"] == residue[1]) & (s["icode"] == " ")
    return s["xyz"][sel] + shift


def _packed_atoms(s, residues, shift):
    """all ATOM records of the residues, residue after residue -> (atoms (n, 3) float64, {residue: (first, end)})"""
    rows, where, n = [], {}, 0
    for res in residues:
        xyz = _residue_atoms(s, res, shift)
        where[res] = (n, n + len(xyz))
        rows.append(xyz)
        n += len(xyz)
    return (np.concatenate(rows) if rows else np.zeros((0, 3))), where


class NativeReference(object):
    """What the evaluation kernels need of one target, and the host-side pieces it was built from.
    For the kernels: ``moments`` (nI + 1, 48) float64 and ``counts`` (host) -- ops.native_moments; ``rec_atoms`` / ``lig_atoms``
    float32, the interface atoms of the unbound structures in the docking frame / the ligand's own frame, residue-contiguous;
    ``ranges`` (C, 4) int32 with its host copy ``ranges_host``; ``C``; ``contact_dist``.  On the host: ``interfaces`` (the
    selections of ``unbound_interfaces``), ``pairs`` (the interface point sets), ``ligand_ca`` / ``target_ca`` (the points of the
    ligand RMSD), ``superposition`` (Q, s: bound frame -> docking frame), ``contacts`` (the transferred residue pairs) and
    ``rec_atoms64`` / ``lig_atoms64``.  ``to(device)`` moves the first group.
    Built with ``all_contacts`` it also carries ``all``, the tables of ops.contact_tables (every atom of both structures,
    residue offsets, bounding spheres, the native pairs as a bitmap) for ops.pose_contact_counts; ``to`` moves them too."""

    def __init__(self, **kw):
        self.all = None
        self.__dict__.update(kw)
        self.device = torch.device("cpu")
        self.moments = torch.from_numpy(self.moments_host)
        self.rec_atoms = torch.from_numpy(self.rec_atoms64.astype(np.float32))
        self.lig_atoms = torch.from_numpy(self.lig_atoms64.astype(np.float32))
        self.ranges = torch.from_numpy(self.ranges_host)

    def to(self, device):
        for name in ("moments", "rec_atoms", "lig_atoms", "ranges"):
            setattr(self, name, getattr(self, name).to(device))
        if self.all is not None:
            for name in ALL_CONTACT_TENSORS:
                self.all[name] = self.all[name].to(device)
        self.device = self.moments.device
        return self


ALL_CONTACT_TENSORS = ("rec_atoms", "rec_off", "rec_sph", "lig_atoms", "lig_off", "lig_sph", "native_bits")


def native_reference_from_points(pairs, ligand_ca, target_ca, rec_atoms, lig_atoms, ranges, contact_dist=5.0, all_rec=None,
                                 all_lig=None, all_pairs=None, **host):
    """A ``NativeReference`` from explicit point sets (``native_reference`` without the PDB files): the arguments of
    ops.native_moments, the two interface atom arrays (float64, residue-contiguous) and the contacts' atom ranges (C, 4).
    ``all_rec`` / ``all_lig``: (atoms (n, 3), offsets (nres + 1)) of EVERY atom of the two structures, residue-contiguous, in
    the same frames, and ``all_pairs``: the native pairs as (receptor residue, ligand residue) indices into them -- all three
    or none; with them the reference serves ops.pose_contact_counts."""
    from deeplocalproteindocking_amd import ops
    moments, counts = ops.native_moments(pairs, ligand_ca, target_ca)
    ranges = np.ascontiguousarray(np.asarray(ranges, dtype=np.int32).reshape(-1, 4))
    if (all_rec is None) != (all_lig is None) or (all_rec is None) != (all_pairs is None):
        raise RuntimeError("dlpd: all_rec, all_lig and all_pairs go together")
    tables = None if all_rec is None else ops.contact_tables(all_rec[0], all_rec[1], all_lig[0], all_lig[1], all_pairs)
    host.setdefault("rec_residues", None)                                               # (named by native_reference(all_contacts=True))
    host.setdefault("lig_residues", None)
    return NativeReference(moments_host=moments, counts=counts, rec_atoms64=np.asarray(rec_atoms, dtype=np.float64).reshape(-1, 3),
                           lig_atoms64=np.asarray(lig_atoms, dtype=np.float64).reshape(-1, 3), ranges_host=ranges, C=int(ranges.shape[0]),
                           contact_dist=float(contact_dist), pairs=pairs, ligand_ca=ligand_ca, target_ca=target_ca, all=tables, **host)


def _all_residues(s):
    """the residues ``native_contact_pairs`` sees (standard amino acids, no insertion code), in file order"""
    seen, order = set(), []
    for i in np.nonzero(_standard(s))[0]:
        key = (str(s["chain"][i]), int(s["resnum"][i]))
        if key not in seen:
            seen.add(key)
            order.append(_residue(s, i))
    return order


def _packed_standard_atoms(s, shift):
    """every ATOM record of every residue of ``_all_residues``, residue after residue -> (atoms (n, 3), offsets, {(chain,
    resnum): index})"""
    residues = _all_residues(s)
    rows, off = [], [0]
    for res in residues:
        rows.append(_residue_atoms(s, res, shift))                                      # (as the interface arrays take them)
        off.append(off[-1] + len(rows[-1]))
    atoms = np.concatenate(rows) if rows else np.zeros((0, 3))
    return atoms, np.asarray(off, dtype=np.int32), {(r[0], r[1]): k for k, r in enumerate(residues)}


def native_reference(bound_receptor, bound_ligand, unbound_receptor, unbound_ligand, contact_dist=5.0, all_contacts=False):
    """Everything the evaluation of one target's poses needs (structures as ``read_structure`` gives them, or file names).
    The docking frame: each unbound structure about its own bounding-box centre, the ligand then placed by the pose.
      I-RMSD   the interface pairs of ``unbound_interfaces``, C-alpha, as ``evaluate_target`` selects them;
      L-RMSD   every aligned ligand residue with a C-alpha in both structures; the bound ligand's are carried into the docking
               frame by the Kabsch fit of the bound receptor's aligned C-alphas onto the unbound receptor's;
      fnat     ``native_contact_pairs`` of the bound complex, transferred (``transfer_pairs``); per contact all ATOM records of
               the two unbound residues;
      fnonnat  (``all_contacts``) every ATOM record of every standard residue of the two unbound structures, and the
               transferred contacts as a set over them."""
    br, bl, ur, ul = (read_structure(s) if isinstance(s, str) else s for s in (bound_receptor, bound_ligand, unbound_receptor, unbound_ligand))
    shift_r, shift_l = -bbox_centre(ur), -bbox_centre(ul)
    interfaces = unbound_interfaces(br, bl, ur, ul, contact_dist)
    pairs = []
    for urec_sel, ulig_sel, brec_sel, blig_sel in interfaces:
        pairs.append((select_ca(ur, urec_sel, shift_r).numpy(), select_ca(ul, ulig_sel, shift_l).numpy(),
                      torch.cat([select_ca(br, brec_sel), select_ca(bl, blig_sel)], dim=0).numpy()))
    rec_match, lig_match = best_chain_match(br, ur), best_chain_match(bl, ul)
    b_ca, u_ca = aligned_ca(br, ur, rec_match)
    if len(b_ca) < 3:
        raise Exception("Too few aligned receptor residues for a superposition", len(b_ca))
    Q, s = kabsch_fit(b_ca, u_ca + shift_r)
    bl_ca, ul_ca = aligned_ca(bl, ul, lig_match)
    if len(bl_ca) < 1:
        raise Exception("No aligned ligand residue")
    ligand_ca, target_ca = ul_ca + shift_l, bl_ca @ Q.T + s
    bound_pairs, contacts = transfer_pairs(native_contact_pairs(br, bl, contact_dist), br, ur, rec_match, bl, ul, lig_match)
    rec_atoms, rec_at = _packed_atoms(ur, sorted(set(c[0] for c in contacts)), shift_r)
    lig_atoms, lig_at = _packed_atoms(ul, sorted(set(c[1] for c in contacts)), shift_l)
    ranges = [rec_at[r] + lig_at[l] for r, l in contacts]
    extra = {}
    if all_contacts:
        ra, ro, rindex = _packed_standard_atoms(ur, shift_r)
        la, lo, lindex = _packed_standard_atoms(ul, shift_l)
        extra = dict(all_rec=(ra, ro), all_lig=(la, lo), all_pairs=[(rindex[r[:2]], lindex[l[:2]]) for r, l in contacts],
                     rec_residues=_all_residues(ur), lig_residues=_all_residues(ul))
    return native_reference_from_points(pairs, ligand_ca, target_ca, rec_atoms, lig_atoms, ranges, contact_dist, interfaces=interfaces,
                                        superposition=(Q, s), contacts=contacts, bound_contacts=bound_pairs, **extra)


class ComplexReference(object):
    """What the interface kernels (csrc/dlpd_interface.h) need of one target when there is no native: ``all``, the
    tables of ops.contact_tables over every ATOM record of every standard residue of the two unbound structures (no native
    pairs), in the frames of ``native_reference``; ``rec_residues`` / ``lig_residues``, the residues as (chain, resnum, name)
    in the order of the bitmaps' bits; ``contact_dist``.  ``to(device)`` moves the tables.  A ``NativeReference`` built with
    ``all_contacts=True`` carries the same three and is taken wherever this is."""

    def __init__(self, tables, rec_residues, lig_residues, contact_dist):
        self.all, self.rec_residues, self.lig_residues, self.contact_dist = tables, list(rec_residues), list(lig_residues), float(contact_dist)
        self.device = torch.device("cpu")

    def to(self, device):
        for name in ALL_CONTACT_TENSORS:
            self.all[name] = self.all[name].to(device)
        self.device = self.all["rec_atoms"].device
        return self


def complex_reference(unbound_receptor, unbound_ligand, contact_dist=5.0):
    """The ``ComplexReference`` of two unbound structures (as ``read_structure`` gives them, or file names): each about its own
    bounding-box centre, the ligand then placed by the pose -- the frame of a .dat file."""
    from deeplocalproteindocking_amd import ops
    ur, ul = (read_structure(s) if isinstance(s, str) else s for s in (unbound_receptor, unbound_ligand))
    ra, ro, _ = _packed_standard_atoms(ur, -bbox_centre(ur))
    la, lo, _ = _packed_standard_atoms(ul, -bbox_centre(ul))
    return ComplexReference(ops.contact_tables(ra, ro, la, lo, ()), _all_residues(ur), _all_residues(ul), contact_dist)


def conformation_poses(conformations):
    """``parse_output``'s conformations (truncated translations included) -> (K, 12) float64: R row-major, then t"""
    return np.stack([np.concatenate([R.numpy().reshape(9), t.numpy().reshape(3)]) for R, t, _ in conformations]).astype(np.float64)


def evaluate_target_device(parser, target_name, bound_receptor_pdb, bound_ligand_pdb, unbound_receptor_pdb, unbound_ligand_pdb,
                           num_conf=None, contact_dist=5.0, device="cuda", lib=None):
    """``evaluate_target`` on the device and for all four quantities: every conformation of ``<decoys_dir>/<target_name>.dat``
    (None if the file is missing), poses as ``parse_output`` keeps them, in one call -> dict of numpy arrays ``irmsd``,
    ``lrmsd``, ``fnat`` (float64) and ``capri`` (int32), plus the ``native`` reference they were measured against."""
    from deeplocalproteindocking_amd import ops
    if parser.parse_output(target_name, header_only=False) is None:
        return None
    confs = parser.target_dict["conformations"]
    n = len(confs) if num_conf is None else min(len(confs), int(num_conf))
    native = native_reference(bound_receptor_pdb, bound_ligand_pdb, unbound_receptor_pdb, unbound_ligand_pdb, contact_dist).to(device)
    out = {"irmsd": np.zeros(0), "lrmsd": np.zeros(0), "fnat": np.zeros(0), "capri": np.zeros(0, dtype=np.int32), "native": native}
    if n:
        got = ops.pose_evaluate(conformation_poses(confs[:n]), native, lib=lib)
        out.update({k: v.cpu().numpy() for k, v in zip(("irmsd", "lrmsd", "fnat", "capri"), got)})
    return out
