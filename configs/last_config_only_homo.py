"""configs/last_config.py with only_homo=True: train_eval_foward stops after the homography (core/flowHomoAdpater.py:115-118),
the UDIS2-homography baseline.  ``python evaluate.py --model_config_name last_config_only_homo``."""
import copy

from configs.last_config import config_dict as _shipped

config_dict = copy.deepcopy(_shipped)
config_dict["only_homo"] = True
