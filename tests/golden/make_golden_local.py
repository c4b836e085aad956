"""Generate tests/golden/local/g8_local_forward.npz by IMPORTING the reference's own code (as make_golden.py does, with the
same stubs for the un-installed TorchProteinLibrary / se3cnn).

Run in the authoring container only (needs the reference tree, where make_golden.py looks for it):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_local.py            # rewrite the fixture
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_local.py --check    # regenerate elsewhere, compare array for array

  G8  src/Models/DockingModels.py   LocalDockingModel.forward (the reference's class, its SimpleFilter and MultiplyVolumes)
      src/Models/ProteinRepresentationModels.py   E3MultiResRepr4x4(multiplier=1), plain torch, seeded state dict (as G7)
      a seeded (B, 11, 12^3) receptor / ligand batch; T rows with negative odd and fractional components and one row with a
      component >= L                                                -> local/g8_local_forward.npz
A sub-folder, because make_golden.py --check walks tests/golden/*.npz.  Only data is written; no reference source is copied.
"""
import importlib
import json
import os
import sys
import tempfile

sys.dont_write_bytecode = True
import numpy as np
import torch

FIXTURES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "local")
NAME = "g8_local_forward.npz"
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def generate(out_dir):
    import make_golden
    make_golden.install_stubs()
    import warnings
    warnings.filterwarnings("ignore")
    DM = importlib.import_module("src.Models.DockingModels")
    PR = importlib.import_module("src.Models.ProteinRepresentationModels")
    torch.manual_seed(801)
    net = PR.E3MultiResRepr4x4(multiplier=1).eval()
    filt = DM.SimpleFilter(net.get_num_outputs()).eval()
    model = DM.LocalDockingModel(net, filt).eval()
    g = torch.Generator().manual_seed(802)
    B, L = 6, 12
    rec = torch.relu(torch.randn(B, 11, L, L, L, generator=g)) * 0.5           # density-like: non-negative
    lig = torch.relu(torch.randn(B, 11, L, L, L, generator=g)) * 0.5
    T = torch.tensor([[0.0, 0.0, 0.0], [-3.0, 5.0, -1.0], [2.5, -4.75, 1.25], [-7.0, -5.0, 3.0], [12.0, 1.0, -2.0],
                      [-0.5, 7.9, -11.0]], dtype=torch.float32)
    with torch.no_grad():
        rv, lv = net(rec), net(lig)
        y = model(rec, lig, T)
    g8 = {"receptor": rec.numpy(), "ligand": lig.numpy(), "T": T.numpy(), "out": y.numpy(),
          "num_outputs": np.array(net.get_num_outputs(), dtype=np.int64)}
    for tag, sd in (("repr", net.state_dict()), ("filter", filt.state_dict())):
        g8[tag + "_keys"] = np.frombuffer(json.dumps(list(sd.keys())).encode(), dtype=np.uint8)
        for k, v in sd.items():
            g8["%s_sd_%s" % (tag, k)] = v.numpy()
    for i in range(len(rv)):
        g8["rec_vol%d" % i], g8["lig_vol%d" % i] = rv[i].numpy(), lv[i].numpy()
    os.makedirs(out_dir, exist_ok=True)
    np.savez_compressed(os.path.join(out_dir, NAME), **g8)
    return os.path.join(out_dir, NAME)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--check":
        fresh = np.load(generate(tempfile.mkdtemp(prefix="dlpd_golden_local_")), allow_pickle=False)
        have = np.load(os.path.join(FIXTURES, NAME), allow_pickle=False)
        same = sorted(have.files) == sorted(fresh.files) and all(
            have[k].dtype == fresh[k].dtype and have[k].shape == fresh[k].shape and np.array_equal(have[k], fresh[k])
            for k in have.files)
        print("%-28s %3d arrays  %s" % (NAME, len(have.files), "identical" if same else "DIFFERENT"))
        sys.exit(0 if same else 1)
    path = generate(FIXTURES)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
