"""``select_model(args)`` as the reference's test driver imports it (local_test.py:14, contract of
/root/reference/src/local_train.py:19-43): the names in ``args.group`` / ``args.model`` /
``args.filter`` pick a representation plugin and a filter, both moved to the GPU.
What the reference's driver builds from them is here too: ``Models.LocalDockingModel`` (made differentiable by the trainer),
``Models.BatchRankingLoss`` and ``Training.LocalTrainer`` (``optimize`` / ``score`` on ``(receptor_files, ligand_files,
labels)``), ``Dataset.get_dataset_stream`` and the epoch loop (``main``; local_train.py:46-118)."""
from Models import E3MultiResRepr4x4, SE3MultiResReprScalar, SimpleFilter, SyntheticRepr

# equivariance group -> {model name -> constructor}
REPRESENTATIONS = {
    "E3": {"E3MultiResRepr4x4": lambda: E3MultiResRepr4x4(multiplier=8)},
    "SE3": {"SE3MultiResReprScalar": lambda: SE3MultiResReprScalar(multiplier=8),
            "SyntheticRepr": lambda: SyntheticRepr(num_outputs=(48,))},
}
FILTERS = {"SimpleFilter": SimpleFilter}


def select_model(args):
    models = REPRESENTATIONS.get(args.group)
    if models is None:
        raise Exception("Unknown equivariance group", args.group)
    if args.model not in models:
        raise Exception("Unknown model name", args.model)
    if args.filter not in FILTERS:
        raise Exception("Unknown filter name", args.filter)
    protein_model = models[args.model]().cuda()
    conformations_filter = FILTERS[args.filter](protein_model.get_num_outputs()).cuda()
    return protein_model, conformations_filter


def _progress(stream):
    try:
        from tqdm import tqdm
    except ImportError:
        return stream
    return tqdm(stream)


def main(argv=None, docking_model=None, lib=None):
    """The reference's epoch loop (local_train.py:46-118) with its arguments, plus what its ``src/__init__.py`` site
    configuration holds there: -data_dir / -log_dir / -models_dir, and -box_size, -resolution, -batch_size, -seed.  Per epoch:
    new_log(training_epoch%d.dat), ``optimize`` over the training stream, ``save``, new_log(validation_epoch%d.dat), ``score``
    over the validation stream, the two mean losses printed.  A batch with fewer than two entries is skipped and counted
    (``BatchRankingLoss`` raises there).  ``docking_model`` / ``lib``: a model built by the caller and the kernel library it
    runs on (the test-suite's emulated one); default: ``select_model(args)`` on the GPU.
    -> {"train": [mean per epoch], "valid": [...], "skipped": batches skipped in all}."""
    import argparse
    import os

    import numpy as np
    import torch
    from Dataset import get_dataset_stream
    from Models import BatchRankingLoss, LocalDockingModel
    from Training import LocalTrainer
    parser = argparse.ArgumentParser(description="Train deep protein docking")
    parser.add_argument("-experiment", default="LocalDebugE3", help="Experiment name")
    parser.add_argument("-group", default="E3", help="Equivariance group of the algorithm", type=str)
    parser.add_argument("-model", default="E3MultiResRepr4x4", help="Name of the model to train", type=str)
    parser.add_argument("-filter", default="SimpleFilter", help="Name of the filter to train", type=str)
    parser.add_argument("-dataset", default="Docking/SplitComplexes:debug_set.dat:debug_set.dat", help="name:training subset:validation subset")
    parser.add_argument("-lr", default=0.0001, help="Learning rate", type=float)
    parser.add_argument("-lrd", default=0.00001, help="Learning rate decay", type=float)
    parser.add_argument("-load_epoch", default=-1, help="Epoch to resume from", type=int)
    parser.add_argument("-max_epoch", default=100, help="Max epoch", type=int)
    parser.add_argument("-data_dir", default="data", help="Where the datasets live (the reference's DATA_DIR)")
    parser.add_argument("-log_dir", default="logs", help="Where the experiment's logs go (LOG_DIR)")
    parser.add_argument("-models_dir", default="models", help="Where the experiment's checkpoints go (MODELS_DIR)")
    parser.add_argument("-box_size", default=80, type=int)
    parser.add_argument("-resolution", default=1.25, type=float)
    parser.add_argument("-batch_size", default=10, type=int)
    parser.add_argument("-seed", default=42, type=int, help="torch.manual_seed, the streams' shuffles and the trainer's rotations")
    args = parser.parse_args(argv)

    torch.manual_seed(args.seed)
    name, subset_train, subset_val = args.dataset.split(":")
    data_dir = os.path.join(args.data_dir, name)
    if docking_model is None:
        torch.cuda.set_device(0)
        protein_model, conformations_filter = select_model(args)
        docking_model = LocalDockingModel(representation=protein_model, filter=conformations_filter).cuda()
    device = next(docking_model.parameters()).device
    stream_train = get_dataset_stream(data_dir, subset=subset_train, field="quality", threshold=1, batch_size=args.batch_size, shuffle=True,
                                      seed=args.seed, device=device)
    stream_valid = get_dataset_stream(data_dir, subset=subset_val, field="quality", threshold=1, batch_size=args.batch_size, shuffle=True,
                                      seed=args.seed + 1, device=device)
    loss = BatchRankingLoss().to(device)
    print("Num model %s parameters:" % args.model, sum(p.numel() for p in docking_model.parameters() if p.requires_grad))
    trainer = LocalTrainer(model=docking_model, loss=loss, lr=args.lr, lr_decay=args.lrd, box_size=args.box_size, resolution=args.resolution,
                           add_zero=True, zero_weight=1.0, add_neg=False, neg_weight=1.0, randomize_rot=True, lib=lib,
                           rotation_seed=args.seed)
    exp_dir, mdl_dir = os.path.join(args.log_dir, args.experiment), os.path.join(args.models_dir, args.experiment)
    os.makedirs(exp_dir, exist_ok=True)
    os.makedirs(mdl_dir, exist_ok=True)
    if args.load_epoch > -1:
        docking_model.load(mdl_dir, epoch=args.load_epoch)
    out = {"train": [], "valid": [], "skipped": 0}
    for epoch in range(args.load_epoch + 1, args.max_epoch):
        print("\nEpoch", epoch)
        trainer.new_log(os.path.join(exp_dir, "training_epoch%d.dat" % epoch))
        losses = []
        for data in _progress(stream_train):
            if len(data[0]) < 2:
                out["skipped"] += 1
                continue
            losses.append(trainer.optimize(data))
        out["train"].append(float(np.mean(losses)) if losses else float("nan"))
        print("Loss training = ", out["train"][-1])
        docking_model.save(mdl_dir, epoch=epoch)
        trainer.new_log(os.path.join(exp_dir, "validation_epoch%d.dat" % epoch))
        losses = []
        for data in _progress(stream_valid):
            if len(data[0]) < 2:
                out["skipped"] += 1
                continue
            losses.append(trainer.score(data))
        out["valid"].append(float(np.mean(losses)) if losses else float("nan"))
        print("Loss validation = ", out["valid"][-1])
    trainer.cleanup()
    if out["skipped"]:
        print("Skipped %d batches of fewer than two decoys" % out["skipped"])
    return out


if __name__ == "__main__":
    main()
