from efa_xray_amd.postprocess.impact import observation_impact
from efa_xray_amd.postprocess.sensitivity import ensemble_sensitivity, observation_targets
from efa_xray_amd.postprocess.verification import ensemble_verification
from efa_xray_amd.postprocess.products import ensemble_products, probability_verification

__all__ = ["observation_impact", "ensemble_sensitivity", "observation_targets", "ensemble_verification", "ensemble_products",
           "probability_verification"]
