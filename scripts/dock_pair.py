"""Dock one receptor/ligand PDB pair the way the reference's local_test.py does (local_test.py:44-71),
without the benchmark table: representation -> exhaustive rotation x translation search -> <out>.dat.

    python scripts/dock_pair.py receptor.pdb ligand.pdb -out pair.dat [-group SE3|E3] [-angle_inc 15]
        [-experiment DIR -load_epoch N]    # optional trained weights (GlobalDockingModel.load)
        [--refine ANGLE[:STEPS[:RADIUS]]]  # SE3: refine the top list over off-set rotations (ANGLE degrees on a
                                           # (2 STEPS + 1)^3 axis-angle lattice, default 1) and translations within
                                           # RADIUS voxels (default 1) -> <out>.refined.dat beside the .dat
        [--minimize STEPS]                 # SE3: descend the score of every pose of the top list in its rotation, at most STEPS
                                           # trials per pose (Docker.minimize) -> <out>.minimized.dat beside the .dat
        [--minimize-translation]           # with --minimize: a rigid-body descent, the translation moves by fractions of a voxel
                                           # too (Docker.minimize(translation=True)); the .dat carries T + s times the resolution
        [--cluster RADIUS[:KEEP]]          # SE3: cluster the LAST list the run produced (the top list, or the refined / minimised
                                           # one) by pose RMSD over the ligand's atoms, greedily in score order, RADIUS in Angstrom,
                                           # at most KEEP clusters (Docker.cluster) -> <out>.clustered.dat (the centres) and
                                           # <out>.clustered.sizes.txt (their populations, one per line) beside the .dat
        [--native BOUND_REC.pdb BOUND_LIG.pdb]  # evaluate every pose against the native complex (Docker.evaluate: interface RMSD,
                                           # ligand RMSD, fraction of native contacts, CAPRI class; receptor.pdb / ligand.pdb are
                                           # the unbound structures) -> <out>.eval.txt, one line per pose of the .dat, and a
                                           # summary; likewise <out>.refined.eval.txt / .minimized.eval.txt / .clustered.eval.txt
                                           # for the lists of the steps that ran
        [--restraint REC_SEL LIG_SEL DMAX[:DMIN]]...   # distance restraints of the search (build-defined): the atom selected in
                                           # the receptor file ("CHAIN:RESNUM[:ATOM]", CA by default, * = the residue's
                                           # centroid, _ = blank chain) lies within [DMIN, DMAX] Angstrom of the one selected
                                           # in the ligand file; only poses that satisfy them enter the list
        [--restraints-needed M]            # ... at least M of them (default: all)
        [--exclusion R]                    # exclusion radius of the search in voxels (0..4, default 0 = the reference's list): a
                                           # rotation contributes only the voxels that nothing within R voxels beats
                                           # (Docker(exclusion=R), build-defined), so the list holds distinct minima instead of
                                           # the neighbours of a few; every later step takes that list as it is
        [--decoys DIR[:NEAR[:FAR]]]        # with --native: write a training set for this target under DIR in the layout
                                           # Dataset.get_dataset_stream reads (Dataset.DecoySet): NEAR poses round the native one
                                           # (default 10) and the first FAR poses (default 10) of the list the run ends with -- the
                                           # clustered one if --cluster was given, else the top list -- each labelled by
                                           # Docker.evaluate(fnonnat=True); the target is named after <out>
        [--interface [N][:boltzmann:T | :rank]]  # which residues of each protein the top list puts in the interface
                                           # (Docker.interface: a residue counts for a pose when one of its atoms lies within 5 A
                                           # of the partner; weights uniform, or Boltzmann in the score at temperature T, or
                                           # 1 / (1 + position)) -> <out>.interface.txt (side, chain, residue, name, count,
                                           # frequency per line) and the N (default 10) most frequent residues of each side as
                                           # CHAIN:RESNUM, the form --restraint takes
        [--cluster-interface THRESHOLD[:KEEP]]  # cluster the top list by the similarity of the poses' interfaces: two poses are
                                           # neighbours when the Jaccard index of their residue sets is >= THRESHOLD (0..1)
                                           # (Docker.cluster_interface) -> <out>.iclustered.dat and <out>.iclustered.sizes.txt

Multi-GPU: launch with torch.distributed.run; rotations are sharded over the ranks, rank 0 writes."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import __graft_entry__ as entry


def parse_cluster(spec):
    """RADIUS[:KEEP] -> (radius in Angstrom, keep or None)"""
    part = spec.split(":")
    return float(part[0]), (int(part[1]) if len(part) > 1 and part[1] else None)


def parse_exclusion(spec):
    """R -> the exclusion radius in voxels, 0 (none) .. 4"""
    r = int(spec)
    if not 0 <= r <= 4:
        raise ValueError("--exclusion takes 0 (none, the reference's list) .. 4 voxels, got %r" % (spec,))
    return r


def parse_restraint_distance(spec):
    """DMAX[:DMIN] -> (dmax, dmin) in Angstrom"""
    part = str(spec).split(":")
    dmax, dmin = float(part[0]), (float(part[1]) if len(part) > 1 and part[1] else 0.0)
    if not 0.0 <= dmin <= dmax < float("inf"):
        raise ValueError("--restraint takes DMAX[:DMIN] with 0 <= DMIN <= DMAX, got %r" % (spec,))
    return dmax, dmin


def set_restraints(docker, prepared, restraints, needed=None):
    """``--restraint REC_SEL LIG_SEL DMAX[:DMIN]`` (repeated) and ``--restraints-needed M`` -> ``docker.restraints``: the
    selections are looked up in the pair's two PDB files and mapped into the search frame (``restraints_from_selections``)."""
    if not restraints:
        docker.restraints, docker.restraints_needed = None, None
        return None
    sel = [(r[0], r[1]) + parse_restraint_distance(r[2]) for r in restraints]
    if needed is not None and not 1 <= int(needed) <= len(sel):
        raise ValueError("--restraints-needed takes 1 .. %d (the number of --restraint), got %r" % (len(sel), needed))
    docker.restraints = docker.restraints_from_selections(prepared, sel)
    docker.restraints_needed = None if needed is None else int(needed)
    return docker.restraints


def search(docker, receptor, ligand, group, batch_size, prepared=None, exclusion=0, restraints=None, restraints_needed=None):
    """The search step: ``Docker.dockSE3`` / ``dockE3`` with the exclusion radius of ``--exclusion`` and the restraints of
    ``--restraint`` (they need ``prepared``: its centring shifts place the selections) -> the top list."""
    docker.exclusion = parse_exclusion(exclusion)
    set_restraints(docker, prepared, restraints, restraints_needed)
    (docker.dockSE3 if group == "SE3" else docker.dockE3)(receptor, ligand, batch_size, prepared=prepared)
    return docker.top_list


def cluster_and_write(docker, prepared, out, radius, keep=None, poses=None, rank=0):
    """The --cluster step: ``Docker.cluster_prepared`` on ``poses`` (None: the top list), then <out>.clustered.dat and
    <out>.clustered.sizes.txt written by ``rank`` 0 (every rank clusters the same gathered list)."""
    docker.cluster_prepared(prepared, poses=poses, radius=radius, keep=keep)
    stem = (out[:-4] if out.endswith(".dat") else out) + ".clustered"
    name, sizes_name = stem + ".dat", stem + ".sizes.txt"
    if rank == 0:
        docker.new_log(name, rewrite=True)
        docker.write_clustered_conformations()
        docker.cleanup()
        with open(sizes_name, "w") as f:
            f.write("".join("%d\n" % e[4] for e in docker.clustered_list))
        sizes = [e[4] for e in docker.clustered_list]
        print("wrote", name, "(%d clusters of %d poses, largest %d, best score %f)" %
              (len(sizes), sum(sizes), max(sizes) if sizes else 0, docker.clustered_list[0][2] if sizes else float("nan")))
    return name, sizes_name


def parse_interface(spec):
    """[N][:boltzmann:T | :rank] -> (residues printed per side, weights, temperature or None)"""
    part = str(spec).split(":")
    n = int(part[0]) if part[0] else 10
    if len(part) == 1:
        return n, "uniform", None
    if part[1] == "rank" and len(part) == 2:
        return n, "rank", None
    if part[1] == "boltzmann" and len(part) == 3 and float(part[2]) > 0.0:
        return n, "boltzmann", float(part[2])
    raise ValueError("--interface takes [N][:boltzmann:T | :rank] with T > 0, got %r" % (spec,))


def parse_cluster_interface(spec):
    """THRESHOLD[:KEEP] -> (Jaccard threshold in [0, 1], keep or None)"""
    threshold, keep = parse_cluster(spec)
    if not 0.0 <= threshold <= 1.0:
        raise ValueError("--cluster-interface takes a THRESHOLD in [0, 1], got %r" % (spec,))
    return threshold, keep


def interface_and_write(docker, complex, out, n=10, weights="uniform", temperature=None, poses=None, rank=0):
    """The --interface step: ``Docker.interface`` on ``poses`` (None: the top list), then <out>.interface.txt and the ``n`` most
    frequent residues of each side, by ``rank`` 0 (every rank treats the same gathered list) -> the file's name"""
    prof = docker.interface(complex, poses=poses, weights=weights, temperature=temperature)
    name = (out[:-4] if out.endswith(".dat") else out) + ".interface.txt"
    if rank == 0:
        docker.new_log(name, rewrite=True)
        docker.write_interface()
        docker.cleanup()
        print("wrote", name, "(%d poses; %d receptor and %d ligand residues in some interface)" %
              (prof["K"], int((prof["rec_count"] > 0).sum()), int((prof["lig_count"] > 0).sum())))
        for side in ("receptor", "ligand"):
            print("  %-8s" % side, " ".join(docker.interface_residues(side, n=n)))
    return name


def cluster_interface_and_write(docker, complex, out, threshold, keep=None, poses=None, rank=0):
    """The --cluster-interface step: ``Docker.cluster_interface`` on ``poses`` (None: the top list), then <out>.iclustered.dat
    and <out>.iclustered.sizes.txt written by ``rank`` 0"""
    docker.cluster_interface(complex, poses=poses, threshold=threshold, keep=keep)
    stem = (out[:-4] if out.endswith(".dat") else out) + ".iclustered"
    name, sizes_name = stem + ".dat", stem + ".sizes.txt"
    if rank == 0:
        docker.new_log(name, rewrite=True)
        docker.write_clustered_conformations()
        docker.cleanup()
        sizes = [e[4] for e in docker.clustered_list]
        with open(sizes_name, "w") as f:
            f.write("".join("%d\n" % s for s in sizes))
        print("wrote", name, "(%d interface clusters of %d poses, largest %d)" % (len(sizes), sum(sizes), max(sizes) if sizes else 0))
    return name, sizes_name


def evaluation_summary(ev):
    """The best class and the lowest I-RMSD among the first 1 / 10 / 100 / all poses, and the rank of the first pose of class
    >= 1 (1-based; None: there is none) -> (rows [(n, best class, lowest irmsd)], rank)"""
    K = len(ev["capri"])
    rows = [(n, int(ev["capri"][:n].max()), float(ev["irmsd"][:n].min())) for n in sorted(set(min(m, K) for m in (1, 10, 100, K))) if n]
    hit = [k for k in range(K) if ev["capri"][k] >= 1]
    return rows, (hit[0] + 1 if hit else None)


def evaluate_and_write(docker, native, out, poses=None, tag="", rank=0):
    """The --native step: ``Docker.evaluate`` on ``poses`` (None: the top list), then <out>[.tag].eval.txt (one line per pose:
    irmsd lrmsd fnat capri) and the summary, by ``rank`` 0 (every rank evaluates the same gathered list)."""
    ev = docker.evaluate(native, poses=poses)
    name = (out[:-4] if out.endswith(".dat") else out) + ("." + tag if tag else "") + ".eval.txt"
    if rank == 0:
        docker.new_log(name, rewrite=True)
        docker.write_evaluation()
        docker.cleanup()
        rows, first = evaluation_summary(ev)
        print("wrote", name, "(%d poses against %d native contacts)" % (len(ev["capri"]), native.C))
        for n, cls, irmsd in rows:
            print("  top %-6d best CAPRI class %d, lowest I-RMSD %.3f A" % (n, cls, irmsd))
        print("  first pose of class >= 1:", "rank %d" % first if first else "none")
    return name


def parse_decoys(spec):
    """DIR[:NEAR[:FAR]] -> (dataset directory, poses round the native, poses of the run's last list)"""
    part = spec.split(":")
    return part[0], (int(part[1]) if len(part) > 1 and part[1] else 10), (int(part[2]) if len(part) > 2 and part[2] else 10)


def decoys_and_write(docker, native, dataset_dir, out, receptor, ligand, poses=None, near=10, far=10, seed=0, subset="training_set.dat",
                     rank=0):
    """The --decoys step: ``near`` poses round the native one and the first ``far`` entries of ``poses`` (None: the top list),
    evaluated with ``fnonnat=True`` and written as one target of a training set under ``dataset_dir`` by ``rank`` 0
    -> the path of the target's table."""
    from deeplocalproteindocking_amd.Dataset.DecoySet import near_native_poses, pose_entries, write_decoy_set
    entries = pose_entries(near_native_poses(native, near, seed=seed), docker) if near > 0 else []
    entries += list(docker.top_list if poses is None else poses)[:far]
    ev = docker.evaluate(native, poses=entries, fnonnat=True)
    target = os.path.basename(out[:-4] if out.endswith(".dat") else out)
    if rank != 0:
        return os.path.join(dataset_dir, "Description", "%s.dat" % target)
    table = write_decoy_set(dataset_dir, target, receptor, ligand, docker.dat_frame_poses(entries), ev, subset=subset)
    print("wrote", table, "(%d decoys, %d of class >= 1, fnonnat %.3f .. %.3f)" %
          (len(entries), int((ev["capri"] >= 1).sum()), float(ev["fnonnat"].min()), float(ev["fnonnat"].max())))
    return table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("receptor")
    ap.add_argument("ligand")
    ap.add_argument("-out", default="pair.dat")
    ap.add_argument("-group", default="SE3")
    ap.add_argument("-model", default=None)
    ap.add_argument("-angle_inc", default=15, type=int)
    ap.add_argument("-threshold_clash", default=300.0, type=float)
    ap.add_argument("-box_size", default=80, type=int)
    ap.add_argument("-resolution", default=1.25, type=float)
    ap.add_argument("-max_conf", default=2000, type=int)
    ap.add_argument("-batch_size", default=16, type=int)
    ap.add_argument("-experiment", default=None)
    ap.add_argument("-load_epoch", default=0, type=int)
    ap.add_argument("--refine", default=None, metavar="ANGLE[:STEPS[:RADIUS]]")
    ap.add_argument("--minimize", default=None, type=int, metavar="STEPS")
    ap.add_argument("--minimize-translation", action="store_true")
    ap.add_argument("--cluster", default=None, metavar="RADIUS[:KEEP]")
    ap.add_argument("--native", default=None, nargs=2, metavar=("BOUND_REC.pdb", "BOUND_LIG.pdb"))
    ap.add_argument("--decoys", default=None, metavar="DIR[:NEAR[:FAR]]")
    ap.add_argument("--exclusion", default=0, type=parse_exclusion, metavar="R")
    ap.add_argument("--restraint", default=[], action="append", nargs=3, metavar=("REC_SEL", "LIG_SEL", "DMAX[:DMIN]"))
    ap.add_argument("--restraints-needed", default=None, type=int, metavar="M")
    ap.add_argument("--interface", default=None, nargs="?", const="", type=parse_interface, metavar="[N][:boltzmann:T|:rank]")
    ap.add_argument("--cluster-interface", default=None, type=parse_cluster_interface, metavar="THRESHOLD[:KEEP]")
    args = ap.parse_args()
    if args.restraints_needed is not None and not args.restraint:
        ap.error("--restraints-needed needs --restraint")
    if args.decoys is not None and args.native is None:
        ap.error("--decoys needs --native (the decoys are labelled against the native complex)")
    entry.build()
    from deeplocalproteindocking_amd.Docker import Docker
    from deeplocalproteindocking_amd.Models import (E3MultiResRepr4x4, GlobalDockingModel, SE3MultiResReprScalar,
                                                    SimpleFilter)
    from deeplocalproteindocking_amd.Utils.FullAtom import CoordsBackend
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    torch.cuda.set_device(dev)
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", device_id=dev)
    repr_ = (SE3MultiResReprScalar if args.group == "SE3" else E3MultiResRepr4x4)(multiplier=8)
    model = GlobalDockingModel(repr_, SimpleFilter(repr_.get_num_outputs()), threshold_clash=args.threshold_clash)
    if args.experiment:
        model.load(args.experiment, args.load_epoch)
    model = model.to(dev)
    docker = Docker(model, angle_inc=args.angle_inc, box_size=args.box_size, resolution=args.resolution,
                    max_conf=args.max_conf, device=dev, coords_backend=CoordsBackend(), rank=rank, world_size=world)
    if rank == 0:
        docker.new_log(args.out, rewrite=True)
    refine = None
    if args.refine is not None:
        if args.group != "SE3":
            ap.error("--refine needs -group SE3 (the ligand's volumes are rotated, not re-represented)")
        part = args.refine.split(":")
        refine = (float(part[0]), int(part[1]) if len(part) > 1 else 1, int(part[2]) if len(part) > 2 else 1)
    if args.minimize_translation and args.minimize is None:
        ap.error("--minimize-translation needs --minimize STEPS")
    if args.minimize is not None and args.group != "SE3":
        ap.error("--minimize needs -group SE3 (the ligand's volumes are rotated, not re-represented)")
    if args.cluster is not None and args.group != "SE3":
        ap.error("--cluster needs -group SE3 (the poses move the prepared ligand's atoms)")
    with torch.no_grad():
        prepared = docker.prepare(args.receptor, args.ligand, "SE3") if (refine or args.minimize is not None or args.cluster is not None) else None
        if args.restraint and prepared is None:
            prepared = docker.prepare(args.receptor, args.ligand, args.group)
        search(docker, args.receptor, args.ligand, args.group, args.batch_size, prepared=prepared, exclusion=args.exclusion,
               restraints=args.restraint, restraints_needed=args.restraints_needed)
    docker.cleanup()
    if rank == 0:
        print("wrote", args.out, "(%d poses, %d of them with a negative score, best score %f)" %
              (len(docker.top_list), sum(e[4] < 0 for e in docker.top_list), docker.top_list[0][4]))
    native = None
    if args.native is not None:
        from deeplocalproteindocking_amd.Results.InterfaceSelection import native_reference
        native = native_reference(args.native[0], args.native[1], args.receptor, args.ligand, all_contacts=args.decoys is not None).to(dev)
        evaluate_and_write(docker, native, args.out, rank=rank)
    if refine:
        from deeplocalproteindocking_amd.Utils.Rotations import local_perturbations
        docker.refine_prepared(prepared, perturbations=local_perturbations(refine[0], refine[1]), radius=refine[2])
        if rank == 0:           # every rank refined the same gathered list
            name = (args.out[:-4] if args.out.endswith(".dat") else args.out) + ".refined.dat"
            docker.new_log(name, rewrite=True)
            docker.write_refined_conformations()
            docker.cleanup()
            print("wrote", name, "(%d poses, best score %f)" % (len(docker.refined_list), docker.refined_list[0][2]))
        if native is not None:
            evaluate_and_write(docker, native, args.out, poses=docker.refined_list, tag="refined", rank=rank)
    if args.minimize is not None:
        docker.minimize_prepared(prepared, steps=args.minimize, translation=args.minimize_translation)
        if rank == 0:           # every rank minimised the same gathered list
            name = (args.out[:-4] if args.out.endswith(".dat") else args.out) + ".minimized.dat"
            docker.new_log(name, rewrite=True)
            docker.write_refined_conformations()
            docker.cleanup()
            print("wrote", name, "(%d poses, best score %f)" % (len(docker.refined_list), docker.refined_list[0][2]))
        if native is not None:
            evaluate_and_write(docker, native, args.out, poses=docker.refined_list, tag="minimized", rank=rank)
    if args.cluster is not None:
        radius, keep = parse_cluster(args.cluster)
        last = docker.refined_list if (refine or args.minimize is not None) else None       # (None: the top list)
        cluster_and_write(docker, prepared, args.out, radius, keep, poses=last, rank=rank)
        if native is not None:
            evaluate_and_write(docker, native, args.out, poses=docker.clustered_list, tag="clustered", rank=rank)
    if args.decoys is not None:
        ddir, near, far = parse_decoys(args.decoys)
        decoys_and_write(docker, native, ddir, args.out, args.receptor, args.ligand,
                         poses=docker.clustered_list if args.cluster is not None else None, near=near, far=far, rank=rank)
    if args.interface is not None or args.cluster_interface is not None:      # (last: --cluster-interface replaces clustered_list)
        from deeplocalproteindocking_amd.Results.InterfaceSelection import complex_reference
        complex_ = complex_reference(args.receptor, args.ligand).to(dev)
        if args.interface is not None:
            interface_and_write(docker, complex_, args.out, *args.interface, rank=rank)
        if args.cluster_interface is not None:
            cluster_interface_and_write(docker, complex_, args.out, args.cluster_interface[0], args.cluster_interface[1], rank=rank)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
