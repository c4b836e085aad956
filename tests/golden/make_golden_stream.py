"""Generate tests/golden/g9_training_data.json by IMPORTING the reference's own code (the authoring container only: it needs
/root/reference), under the stubbing make_golden.py uses for the packages that are not installed:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_stream.py            # rewrite the fixture
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_stream.py --check    # regenerate and compare with the committed one

  G9a  scripts/Dataset/processing_utils.py    _get_fnat on sets of given sizes            -> "fnat_cases"
  G9b  src/Dataset/SplitComplexDataset.py     SplitComplexDataset (the parsed tables) and BatchSamplerQuality (its index
                                              batches, shuffle=False, batch sizes 4 and 10, thresholds 1 and 2) on a tiny
                                              dataset written here as text                  -> "dataset", "parsed", "batches"
Only data (inputs and expected outputs) is written; no reference source is copied.  ``__getitem__`` is not recorded: it
creates its label on 'cuda'."""
import importlib
import importlib.util
import json
import os
import sys
import tempfile
import types
from unittest.mock import MagicMock

sys.dont_write_bytecode = True

FIXTURES = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
NAME = "g9_training_data.json"

# (n_nat, n_dec, n_corr): empty sets, no overlap, full overlap, and sizes in between
FNAT_SIZES = [(0, 0, 0), (10, 0, 0), (0, 7, 0), (1, 1, 1), (1, 1, 0), (40, 55, 0), (40, 40, 40), (40, 55, 13), (719, 909, 719), (65, 3, 2),
              (300, 1401, 299), (1000, 999, 501)]

ELSEWHERE = "/data/elsewhere/SplitComplexes"          # the root the tables were written under: a reader re-roots the paths


def install_stubs():
    for name in ["TorchProteinLibrary", "TorchProteinLibrary.FullAtomModel", "TorchProteinLibrary.FullAtomModel.CoordsTransform",
                 "TorchProteinLibrary.Volume", "_Volume", "se3cnn", "se3cnn.non_linearities", "se3cnn.blocks", "se3cnn.filter", "Bio", "Bio.PDB",
                 "Bio.PDB.Polypeptide"]:
        sys.modules[name] = MagicMock()
    sys.modules["prody"] = types.ModuleType("prody")
    src = types.ModuleType("src")
    src.__path__ = [os.path.join(REF, "src")]
    src.REPOSITORY_DIR = REF
    src.DATA_DIR = os.path.join(REF, "data")
    sys.modules["src"] = src


def dataset_text():
    """three targets: no positive decoy (and more decoys than a batch of 10), fewer decoys than a batch, a single decoy"""
    header = "receptor\tligand\tlrmsd\tirmsd\tfnat\tfnonnat\tquality\n"

    def row(t, k, l, i, f, g, q):
        return "%s/Decoys/%s_r.pdb\t%s/Decoys/%s_l_%d.pdb\t%f\t%f\t%f\t%f\t%d\n" % (ELSEWHERE, t, ELSEWHERE, t, k, l, i, f, g, q)
    tables = {
        "1ABC": header + "".join(row("1ABC", k, 20.0 + k, 11.0 + 0.5 * k, 0.01 * k, 0.9 + 0.005 * k, 0) for k in range(12)),
        "2XYZ": header + "".join(row("2XYZ", k, l, i, f, g, q) for k, (l, i, f, g, q) in enumerate(
            [(4.1, 1.9, 0.41, 0.35, 2), (31.0, 14.2, 0.0, 1.0, 0), (8.7, 3.6, 0.18, 0.62, 1), (0.8, 0.6, 0.83, 0.11, 3), (25.5, 12.0, 0.03, 0.97, 0),
             (2.2, 1.1, 0.6, 0.2, 2), (9.9, 3.9, 0.12, 0.7, 1)])),
        "3ONE": header + row("3ONE", 0, 0.5, 0.4, 0.9, 0.1, 3),
    }
    return {"subset": "1ABC\n2XYZ\n3ONE\n", "subset_name": "tiny_set.dat", "tables": tables}


def generate():
    install_stubs()
    spec = importlib.util.spec_from_file_location("ref_processing_utils", os.path.join(REF, "scripts", "Dataset", "processing_utils.py"))
    pu = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(pu)
    cases = []
    for n_nat, n_dec, n_corr in FNAT_SIZES:
        nat = set(("n", i) for i in range(n_nat))
        dec = set(("n", i) for i in range(n_corr)) | set(("d", i) for i in range(n_dec - n_corr))
        fnat, fnonnat = pu._get_fnat(nat, dec)
        cases.append({"n_nat": n_nat, "n_dec": n_dec, "n_corr": n_corr, "fnat": float(fnat), "fnonnat": float(fnonnat)})
    scd = importlib.import_module("src.Dataset.SplitComplexDataset")
    data = dataset_text()
    root = tempfile.mkdtemp(prefix="dlpd_g9_")
    os.makedirs(os.path.join(root, "Description"))
    with open(os.path.join(root, "Description", data["subset_name"]), "w") as f:
        f.write(data["subset"])
    for t, text in data["tables"].items():
        with open(os.path.join(root, "Description", t + ".dat"), "w") as f:
            f.write(text)
    ds = scd.SplitComplexDataset("quality", 1, root, description_set=data["subset_name"])
    parsed = {t: [{k: (os.path.relpath(v, root) if isinstance(v, str) else v) for k, v in row.items()} for row in ds.decoys[t]] for t in ds.targets}
    batches = {}
    for bs in (4, 10):
        for thr in (1, 2):
            sampler = scd.BatchSamplerQuality(ds.targets, ds.decoys, "quality", thr, bs, shuffle=False)
            batches["%d:%d" % (bs, thr)] = [[list(p) for p in b] for b in sampler]
            assert len(sampler) == len(ds.targets)
    return {"fnat_cases": cases, "dataset": data, "targets": list(ds.targets), "size": len(ds), "parsed": parsed, "batches": batches}


def main():
    fresh = generate()
    path = os.path.join(FIXTURES, NAME)
    if "--check" in sys.argv:
        with open(path) as f:
            same = json.load(f) == json.loads(json.dumps(fresh))
        print("%-28s %s" % (NAME, "identical" if same else "DIFFERENT"))
        sys.exit(0 if same else 1)
    with open(path, "w") as f:
        json.dump(fresh, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
