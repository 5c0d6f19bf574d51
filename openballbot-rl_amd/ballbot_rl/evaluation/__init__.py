"""Policy evaluation (reference ballbot_rl/evaluation)."""
from ballbot_rl.evaluation.evaluate import DeviceEvaluator, evaluate_policy
from ballbot_rl.evaluation.sb3_zip import (load_sb3_policy, read_sb3_zip, save_sb3_policy_pth, sb3_state_dict)

__all__ = ["evaluate_policy", "DeviceEvaluator", "read_sb3_zip", "load_sb3_policy", "sb3_state_dict",
           "save_sb3_policy_pth"]
