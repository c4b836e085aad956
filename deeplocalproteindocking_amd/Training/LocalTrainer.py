"""The trainer of the local docking model, with the reference's surface (src/Training/LocalTrainer.py:20-177): constructor
keywords and defaults, ``new_log`` / ``cleanup``, ``load_batch``, ``optimize(data)`` and ``score(data)``, and the same log
lines.  ``data`` is the tuple ``(receptor_files, ligand_files, labels)`` a batch of the reference's dataset stream holds.

What differs is where the arithmetic runs: the atom front end is this build's ``Utils.FullAtom.CoordsBackend`` (in place of
TorchProteinLibrary's PDB2CoordsUnordered / CoordsRotate / Coords2TypedCoords / getBBox / CoordsTranslate /
TypedCoords2Volume), and the model's correlation and its backward are the HIP kernels of csrc/dlpd_local.h and
csrc/dlpd_local_grad.h.  The representation's Conv3d layers train on torch's own kernels by default; ``hip_conv=True``
sends their stride-1 convolutions, forward and backward, through the HIP kernels as well (``ops.conv3d_autograd``,
csrc/dlpd_conv_grad.h) -- the max-pool and a stride-2 layer stay on torch."""
import atexit

import torch
from torch import optim
from torch.optim.lr_scheduler import LambdaLR

from deeplocalproteindocking_amd.Docker.Docker import random_rotation
from deeplocalproteindocking_amd.Utils.Conventions import VolumeConventions
from deeplocalproteindocking_amd.Utils.FullAtom import CoordsBackend


class LocalTrainer:
    def __init__(self, model, loss, lr=0.001, lr_decay=0.0001, box_size=120, resolution=1.0, add_neg=False, neg_weight=0.5,
                 add_zero=False, zero_weight=1.0, randomize_rot=True, lib=None, conventions=None, rotation_seed=None,
                 hip_conv=False):
        """lib: None -> the product library (GPU); the test-suite passes the emulated one (host tensors).  conventions: a
        ``Utils.Conventions.VolumeConventions`` (or the path of its JSON) for the projection's density shape and atom typing,
        as ``Docker`` takes it.  rotation_seed: makes the random rotations reproducible (None: as ``Docker.random_rotation``).
        hip_conv: True sets ``hip_autograd`` on ``model.representation`` when it has that attribute (both plugins do): its
        convolutions then train on the HIP kernels; False leaves the representation as it is."""
        self.lr = lr
        self.lr_decay = lr_decay
        self.model = model
        self.loss = loss
        self.hip_conv = bool(hip_conv)
        representation = getattr(self.model, "representation", None)
        if self.hip_conv and hasattr(representation, "hip_autograd"):
            representation.hip_autograd = True
        # the reference's driver builds LocalDockingModel(representation=, filter=) without a flag: the trainer is what makes
        # it the differentiable model
        if hasattr(self.model, "differentiable"):
            self.model.differentiable = True
        self.optimizer = optim.Adam(self.model.parameters(), lr=self.lr)
        self.log = None
        self.lr_scheduler = LambdaLR(self.optimizer, lambda epoch: 1.0 / (1.0 + epoch * self.lr_decay))

        # zero-score condition
        self.add_zero = add_zero
        self.zero_weight = zero_weight

        # negative-score condition
        self.add_neg = add_neg
        self.neg_weight = neg_weight

        self.box_length = box_size * resolution
        self.box_size = box_size
        self.resolution = resolution

        if isinstance(conventions, str):
            conventions = VolumeConventions.load(conventions)
        self.conventions = conventions.copy() if conventions is not None else VolumeConventions()
        self._lib = lib
        self.coords_backend = CoordsBackend(lib=lib, splat=self.conventions.splat, atom_types=self.conventions.atom_types)

        self.randomize_rot = randomize_rot
        # one generator for the trainer's whole life: seeded, or from the environment / the operating system's entropy as
        # Docker.random_rotation documents
        self._generator = None
        if rotation_seed is not None:
            self._generator = torch.Generator()
            self._generator.manual_seed(int(rotation_seed))

        atexit.register(self.cleanup)

    @property
    def device(self):
        """Where the model lives (the reference hard-codes 'cuda'; the emulated library of the tests runs on host tensors)."""
        for p in self.model.parameters():
            return p.device
        return torch.device("cpu" if self._lib is not None else "cuda")

    def new_log(self, log_file_name):
        if self.log is not None:
            self.log.close()
        self.log = open(log_file_name, "w")

    def cleanup(self):
        if self.log is not None:
            self.log.close()
            self.log = None

    def random_rotations(self, batch_size):
        """(B, 3, 3) float64: one uniform random rotation per batch entry (getRandomRotation(batch_size), LocalTrainer.py:100)."""
        return torch.cat([random_rotation(generator=self._generator) for _ in range(batch_size)], dim=0)

    def load_batch(self, filenames, random_rotations=None):
        """LocalTrainer.py:66-79 through the coords backend -> (volume (B, 11, L, L, L), translation / resolution, a, b)."""
        be = self.coords_backend
        with torch.no_grad():
            coords, _, resnames, resnums, atomnames, num_atoms = be.pdb2coords(filenames)
            if random_rotations is not None:
                coords = be.rotate(coords, random_rotations, num_atoms)
            coords, num_atoms_of_type, offsets = be.assign_types(coords, resnames, atomnames, num_atoms)
            num_atoms = getattr(be, "last_num_typed", num_atoms)        # untyped atoms (hydrogens) were dropped
            a, b = be.get_bbox(coords, num_atoms)
            translation = -(a + b) * 0.5 + self.box_length / 2.0
            coords = be.translate(coords, translation, num_atoms)
            volume = be.project(coords, num_atoms_of_type, offsets, self.box_size, self.resolution, self.device)
        return volume, translation / self.resolution, a, b

    def _load_pair(self, receptor_list, ligand_list):
        """Both batches under ONE rotation per entry, and T = T1 - T2 (LocalTrainer.py:98-107,159-167)."""
        with torch.no_grad():
            rotations = self.random_rotations(len(receptor_list)) if self.randomize_rot else None
            receptor, T1, _, _ = self.load_batch(receptor_list, rotations)
            ligand, T2, _, _ = self.load_batch(ligand_list, rotations)
            T = (T1 - T2).to(receptor.device)
        return receptor, ligand, T

    def _write_log(self, header, receptor_list, ligand_list, model_out, labels):
        self.log.write("Loss\t%f\t%f\t%f\t%f\t%f\n" % header)
        for i in range(len(receptor_list)):
            self.log.write("%s\t%s\t%f\t%f\n" % (receptor_list[i], ligand_list[i], model_out[i].item(), labels[i].item()))

    def optimize(self, data):
        """Optimization step.  Input: data = (receptor files, ligand files, labels).  Output: the loss."""
        self.model.train()
        self.optimizer.zero_grad()

        receptor_list, ligand_list, labels = data
        receptor_list = list(receptor_list)
        ligand_list = list(ligand_list)
        labels = torch.as_tensor(labels).reshape(-1)

        receptor, ligand, T = self._load_pair(receptor_list, ligand_list)

        # ranking interactions
        model_out = self.model(receptor, ligand, T).reshape(-1)
        labels = labels.to(model_out.device)
        L_decoys = self.loss(model_out, labels)
        L = L_decoys

        # interacting decoys should score < 0
        if self.add_neg:
            L_neg = torch.mean(torch.relu(model_out))
            L = L + self.neg_weight * L_neg

        # non-interaction
        if self.add_zero:
            input_zero = torch.zeros(1, self.model.filter.fc_input_size, device=model_out.device, dtype=torch.float)
            output_zero = self.model.filter.fc(input_zero)
            L_zero = torch.abs(output_zero)
            L = L + self.zero_weight * L_zero

        # (the reference raises this where it writes the log line, LocalTrainer.py:136-137; here: log or no log, before the step)
        if self.add_neg and not self.add_zero:
            raise Exception("Stupid choice of the loss function(neg/zero): ", self.add_neg, self.add_zero)

        L.backward()

        if self.log is not None:
            self._write_log((L.item(), L_decoys.item(), 0.0, L_neg.item() if self.add_neg else 0.0,
                             L_zero.item() if self.add_zero else 0.0), receptor_list, ligand_list, model_out, labels)

        self.optimizer.step()
        self.lr_scheduler.step()
        return L.item()

    def score(self, data):
        """Scoring of the data (eval mode, no graph).  Input: data.  Output: the ranking loss."""
        self.model.eval()
        receptor_list, ligand_list, labels = data
        receptor_list = list(receptor_list)
        ligand_list = list(ligand_list)
        labels = torch.as_tensor(labels).reshape(-1)

        receptor, ligand, T = self._load_pair(receptor_list, ligand_list)

        with torch.no_grad():
            model_out = self.model(receptor, ligand, T).reshape(-1)
            labels = labels.to(model_out.device)
            L = self.loss(model_out, labels)

        if self.log is not None:
            self._write_log((L.item(), L.item(), 0.0, 0.0, 0.0), receptor_list, ligand_list, model_out, labels)

        return L.item()
