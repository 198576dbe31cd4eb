from efa_xray_amd.postprocess.impact import observation_impact
from efa_xray_amd.postprocess.sensitivity import ensemble_sensitivity, observation_targets
from efa_xray_amd.postprocess.verification import ensemble_verification
from efa_xray_amd.postprocess.products import ensemble_products, probability_verification
from efa_xray_amd.postprocess.neighbourhood import neighbourhood_probabilities, fractions_skill_score, fss_from_sums
from efa_xray_amd.postprocess.pmmean import probability_matched_mean
from efa_xray_amd.postprocess.modes import (ensemble_gram, ensemble_eofs, ensemble_clusters, distances_from_gram,
                                            eofs_from_gram, clusters_from_gram)

__all__ = ["observation_impact", "ensemble_sensitivity", "observation_targets", "ensemble_verification", "ensemble_products",
           "probability_verification", "ensemble_gram", "ensemble_eofs", "ensemble_clusters", "distances_from_gram",
           "eofs_from_gram", "clusters_from_gram", "neighbourhood_probabilities", "fractions_skill_score", "fss_from_sums",
           "probability_matched_mean"]
