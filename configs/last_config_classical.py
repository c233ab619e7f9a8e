"""configs/last_config.py without reading a single weight: the corner offsets come from corners, binary descriptors and RANSAC
(homo_source="features", stitch_amd/feature_align.py) and the residual flow from a coarse-to-fine Lucas-Kanade (flow_source="dense_lk",
stitch_amd/dense_flow.py).  only_homo stays off and the forward-backward consistency mask stays as shipped, so test_eval and test_out
run their whole path: flow warp, range map, occlusion mask, opening and blend.  ``python evaluate.py --model_config_name
last_config_classical`` is the classical baseline beside last_config_features (the homography alone); ``python out.py
--model_config_name last_config_classical`` stitches without a checkpoint."""
import copy

from configs.last_config import config_dict as _shipped

config_dict = copy.deepcopy(_shipped)
config_dict["homo_source"] = "features"
config_dict["flow_source"] = "dense_lk"
