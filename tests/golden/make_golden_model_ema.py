"""Golden ModelEMA states from the reference's OWN two classes (authoring container only: needs /root/reference; never run by a test).

``ModelEMA`` of det/yolox/utils/ema.py and of lib/torch_utils/torch_utils.py are imported from the reference's files through
``_refimport`` and run UNMODIFIED on the CPU over tests/model_ema_ref.py's small seeded model (Conv2d + BatchNorm2d + Linear + one fp64
buffer).  The packages above the detector's file import the whole trainer and are kept from running: ``det``, ``det.yolox`` and
``det.yolox.utils`` are registered as bare packages.  ``lib.utils.setup_logger`` (``log_first_n``) and ``lib.utils.utils`` (``iprint``)
are served by stand-ins: neither is called on the path taken here; torchvision is one of ``_refimport``'s inert roots.

Per decay (0.9998, 0.9999) and class: a fresh EMA through updates 1..5, and an EMA resumed with ``updates=1999`` through 2000 and 2001;
the model's weights move by seeded noise before each update (``perturb``).
-> model_ema_golden.npz: the model's state before each update, the EMA's state after it, and the decay ``d`` the class used, as fp64."""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", ".."))
import _refimport  # noqa: E402

from tests import model_ema_ref as R  # noqa: E402


def import_reference():
    _refimport.install()
    for pkg in ("det", "det.yolox", "det.yolox.utils"):
        m = types.ModuleType(pkg)
        m.__path__ = [os.path.join(_refimport.REF, *pkg.split("."))]
        sys.modules[pkg] = m
    logger = types.ModuleType("lib.utils.setup_logger")
    logger.log_first_n = lambda *a, **k: None
    utils = types.ModuleType("lib.utils.utils")
    utils.iprint = print
    import lib.utils  # noqa: F401  (the reference's package, so that the two stand-ins hang under it)
    sys.modules["lib.utils.setup_logger"], sys.modules["lib.utils.utils"] = logger, utils
    import det.yolox.utils.ema as yolox_ema
    import lib.torch_utils.torch_utils as gdrn_tu
    for mod, rel in ((yolox_ema, "det/yolox/utils/ema.py"), (gdrn_tu, "lib/torch_utils/torch_utils.py")):
        assert os.path.samefile(mod.__file__, os.path.join(_refimport.REF, rel)), mod.__file__
    return {"yolox": yolox_ema.ModelEMA, "gdrn": gdrn_tu.ModelEMA}


def main():
    import torch

    classes = import_reference()
    assert tuple(classes) == R.CLASSES
    layout = R.build_tiny().state_dict()
    keys = list(layout)
    rec = dict(keys=np.array(keys), dtypes=np.array([str(v.numpy().dtype) for v in layout.values()]),
               shapes=np.array([",".join(map(str, v.shape)) for v in layout.values()]),
               torch_version=np.array(torch.__version__), cpu_capability=np.array(torch.backends.cpu.get_cpu_capability()))

    def flat(state):
        """One fp64 vector per state, entries in key order: fp32, fp64 and the small int64 counter are all exact in fp64."""
        out = np.concatenate([np.asarray(state[k]).astype(np.float64).reshape(-1) for k in keys])
        back = R.unflatten(out, keys, rec["dtypes"], rec["shapes"])
        assert all(np.array_equal(back[k], state[k], equal_nan=True) and back[k].dtype == np.asarray(state[k]).dtype for k in keys)
        return out

    for cls, ModelEMA in classes.items():
        for decay in R.DECAYS:
            for run, spec in R.RUNS.items():
                model = R.build_tiny()
                ema = ModelEMA(model, decay, updates=spec["updates"])
                assert not ema.ema.training and all(not p.requires_grad for p in ema.ema.parameters())
                for t in range(1, spec["steps"] + 1):
                    R.perturb(model, run, t)
                    before = {k: v.detach().clone().numpy() for k, v in model.state_dict().items()}
                    ema.update(model)
                    assert ema.updates == spec["updates"] + t
                    name, before = f"model/{run}/{t}", flat(before)
                    assert name not in rec or np.array_equal(rec[name], before), name      # one trajectory of the model for all
                    rec[name] = before
                    rec[f"ema/{cls}/{decay}/{run}/{t}"] = flat({k: v.detach().clone().numpy() for k, v in ema.ema.state_dict().items()})
                    rec[f"d/{cls}/{decay}/{run}/{t}"] = np.float64(ema.decay(ema.updates))
                assert int(ema.ema.bn.num_batches_tracked) == R.TRACKED_AT_COPY and ema.ema.scale64.dtype == torch.float64
                print(cls, decay, run, "updates", ema.updates, "d", float(rec[f"d/{cls}/{decay}/{run}/{spec['steps']}"]))
    np.savez_compressed(R.GOLDEN, **rec)
    size = os.path.getsize(R.GOLDEN)
    assert size < (1 << 20), size
    print("wrote model_ema_golden.npz", size, "bytes,", len(rec), "arrays")


if __name__ == "__main__":
    main()
