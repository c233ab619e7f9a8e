"""configs/last_config_classical.py with the oriented, multi-scale feature front end (stitch_amd/feature_align.py, multiscale=True;
README.md, feature_align_ms): the same weight-free path for pairs that are rolled -- landscape against portrait, upside down -- or one zoom
step apart, where the upright single-scale descriptor finds no model and the stitch stays unaligned.  ``python evaluate.py
--model_config_name last_config_classical_ms`` and ``python out.py --model_config_name last_config_classical_ms`` read no checkpoint."""
import copy

from configs.last_config_classical import config_dict as _classical

config_dict = copy.deepcopy(_classical)
config_dict["feature_align"] = dict(multiscale=True)
