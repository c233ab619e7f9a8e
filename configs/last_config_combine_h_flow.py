"""configs/last_config.py with use_combine_h_flow=True and use_fb_consistency_mask=False: train_eval_foward warps image 2 once by
the dense homography flow plus the residual flow (core/flowHomoAdpater.py:144-164).  The reference raises for this switch with
the consistency mask on, so both keys change.  ``python evaluate.py --model_config_name last_config_combine_h_flow``."""
import copy

from configs.last_config import config_dict as _shipped

config_dict = copy.deepcopy(_shipped)
config_dict["use_combine_h_flow"] = True
config_dict["use_fb_consistency_mask"] = False
