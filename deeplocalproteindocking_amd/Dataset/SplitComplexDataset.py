"""The training stream, with the reference's surface (src/Dataset/SplitComplexDataset.py:21-160): ``SplitComplexDataset`` reads
<dataset_dir>/Description/<subset> (target names) and one table per target, ``BatchSamplerQuality`` picks one batch per target
-- up to batch_size / 2 decoys with ``field >= threshold``, then decoys below it, up to batch_size -- and
``get_dataset_stream`` joins them in a ``torch.utils.data.DataLoader``: a batch is ``(receptor files, ligand files, labels
(B, 1))``, what ``Training.LocalTrainer.optimize`` / ``score`` take.  ``Dataset.DecoySet.write_decoy_set`` writes such sets.

BEHAVIOUR CHANGE (README): ``shuffle=True`` permutes each target's decoys with a generator the sampler owns (``seed=``; None:
seeded from the operating system), not with the global ``random`` module seeded to 42 at import as the reference does -- the
``rotation_seed`` precedent.  The indices a batch holds always address the tables in file order.  Labels are created on
``device`` (default: the GPU when there is one, else the CPU) where the reference hard-codes 'cuda'."""
import os

import torch
from torch.utils.data import Dataset


class SplitComplexDataset(Dataset):
    """The decoy tables of a subset: ``targets`` (names, file order), ``decoys`` {target: [row dict]} and ``indexed`` (every row).
    A row maps the header's field names to floats where the text parses as one, else to the path re-rooted under
    ``dataset_dir`` by its last two components."""

    def __init__(self, field, threshold, dataset_dir, description_dir="Description", description_set="datasetDescription.dat", device=None,
                 verbose=True):
        self.dataset_dir = dataset_dir
        self.description_path = os.path.join(dataset_dir, description_dir, description_set)
        self.field = field
        self.threshold = threshold
        self.device = torch.device(device) if device is not None else torch.device("cuda" if torch.cuda.is_available() else "cpu")
        self.targets = []
        with open(self.description_path, "r") as fin:
            for line in fin:
                if line.split():
                    self.targets.append(line.split()[0])
        self.decoys = {}
        self.indexed = []
        for target in self.targets:
            self.decoys[target] = []
            with open(os.path.join(dataset_dir, description_dir, "%s.dat" % target), "r") as fin:
                fields = fin.readline().split()
                for line in fin:
                    sline = line.split()
                    if not sline:
                        continue
                    row = {}
                    for n, name in enumerate(fields):
                        try:
                            row[name] = float(sline[n])
                        except ValueError:
                            part = sline[n].split("/")
                            row[name] = os.path.join(self.dataset_dir, part[-2], part[-1])
                    self.decoys[target].append(row)
                    self.indexed.append(row)
        self.dataset_size = len(self.decoys)
        if verbose:
            print("Dataset file: ", self.dataset_dir)
            print("Dataset size: ", self.dataset_size)

    def __getitem__(self, index):
        """(target index, decoy index) -> (receptor file, ligand file, label (1,) float32 on ``device``)"""
        target_index, decoy_index = index
        decoy = self.decoys[self.targets[target_index]][decoy_index]
        label = torch.zeros(1, dtype=torch.float, device=self.device)
        label[0] = decoy[self.field]
        return decoy["receptor"], decoy["ligand"], label

    def __len__(self):
        return self.dataset_size


class BatchSamplerQuality(object):
    """One batch of (target index, decoy index) per target.  ``shuffle``: every pass first permutes each target's decoys with
    the sampler's own generator; the selection then walks them in that order."""

    def __init__(self, targets, decoys, field, threshold, batch_size, shuffle=False, seed=None):
        self.targets = targets
        self.decoys = decoys
        self.batch_size = batch_size
        self.field = field
        self.threshold = threshold
        self.shuffle = shuffle
        self.generator = torch.Generator()
        if seed is None:
            self.generator.seed()
        else:
            self.generator.manual_seed(int(seed))

    def order(self, target):
        n = len(self.decoys[target])
        return torch.randperm(n, generator=self.generator).tolist() if self.shuffle else list(range(n))

    def select_batch(self, decoys_list, order=None):
        """indices into ``decoys_list``: walking it in ``order`` (default: as it stands), the first batch_size / 2 entries with
        field >= threshold, then entries below it while fewer than batch_size are chosen"""
        order = list(range(len(decoys_list))) if order is None else order
        positive, negative, num_added = [], [], 0
        for idx in order:
            if decoys_list[idx][self.field] >= self.threshold and num_added < (self.batch_size / 2.0):
                positive.append(idx)
                num_added += 1
        for idx in order:
            if decoys_list[idx][self.field] < self.threshold and num_added < self.batch_size:
                negative.append(idx)
                num_added += 1
        return positive + negative

    def __iter__(self):
        for idx, target in enumerate(self.targets):
            yield [(idx, d) for d in self.select_batch(self.decoys[target], self.order(target))]

    def __len__(self):
        return len(self.targets)


def _collate(items):
    receptors, ligands = [it[0] for it in items], [it[1] for it in items]
    labels = torch.stack([it[2] for it in items]) if items else torch.zeros(0, 1)
    return receptors, ligands, labels


def get_dataset_stream(data_dir, subset, batch_size=10, field="quality", threshold=1, shuffle=False, seed=None, device=None):
    dataset = SplitComplexDataset(field, threshold, data_dir, description_set=subset, device=device)
    sampler = BatchSamplerQuality(dataset.targets, dataset.decoys, field, threshold, batch_size, shuffle, seed=seed)
    return torch.utils.data.DataLoader(dataset, batch_sampler=sampler, num_workers=0, collate_fn=_collate)
