"""causal-gen on MI355X: the HVAE image-mechanism / counterfactual hot path of biomedia-mira/causal-gen behind
the reference's own Python surface (``vae.HVAE``, ``dmol.DmolNet``, ``dscm.DSCM``), computed by hand-written
gfx950 HIP kernels in ``libcgen_hip.so`` (C ABI: include/cgen_hip.h).  There is no CPU or ATen fallback: the
model classes raise if the library or a GPU is missing."""
__version__ = "0.1.0"


_LAZY = {"DeviceDataset": "data", "DeviceLoader": "data", "PgmCounterfactual": "pgm_cf", "DevicePGM": "pgm_cf",
         "ChestPredictor": "predictor_resnet", "ChestPredictorTrainStep": "predictor_resnet_train",
         "CfTrainStep": "cf_train"}


def __getattr__(name):  # the data pipeline's and the device PGM's classes, re-exported without importing torch at package import
    if name in _LAZY:
        import importlib

        return getattr(importlib.import_module(__name__ + "." + _LAZY[name]), name)
    raise AttributeError(name)
