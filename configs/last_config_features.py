"""configs/last_config.py without either network: the corner offsets come from corners, binary descriptors and RANSAC
(homo_source="features", stitch_amd/feature_align.py), there is no residual flow (flow_source="zero"), and test_eval stops after the
homography (only_homo=True).  ``python evaluate.py --model_config_name last_config_features`` is a classical baseline beside
last_config_only_homo; ``python out.py --model_config_name last_config_features`` stitches without reading either network's weights."""
import copy

from configs.last_config import config_dict as _shipped

config_dict = copy.deepcopy(_shipped)
config_dict["homo_source"] = "features"
config_dict["flow_source"] = "zero"
config_dict["only_homo"] = True
