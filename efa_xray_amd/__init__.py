"""efa_xray_amd: MI355X-native serial EnSRF assimilation update.

A from-scratch gfx950 implementation of the hot path of lmadaus/efa_xray
(`efa_xray/assimilation`): hand-written HIP kernels behind a C ABI
(`include/efa_hip.h`, `libefa_hip.so`), with the reference's Python surface
(`EnsembleState`, `Observation`, `EnSRF(...).update()`) on top.
"""
from efa_xray_amd.state.ensemble import EnsembleState
from efa_xray_amd.observation.observation import Observation, gaspari_cohn, haversine
from efa_xray_amd.assimilation.assimilation import Assimilation
from efa_xray_amd.assimilation.ensrf import EnSRF
from efa_xray_amd.assimilation.etkf import ETKF
from efa_xray_amd.assimilation.letkf import LETKF, SlabLETKF
from efa_xray_amd.assimilation.letkf_inflation import ColumnInflation
from efa_xray_amd.assimilation.adaptive_inflation import AdaptiveInflation
from efa_xray_amd.assimilation.sampling_error import sampling_error_table
from efa_xray_amd.postprocess.impact import observation_impact
from efa_xray_amd.postprocess.sensitivity import ensemble_sensitivity, observation_targets
from efa_xray_amd.postprocess.verification import ensemble_verification
from efa_xray_amd.postprocess.products import ensemble_products, probability_verification
from efa_xray_amd.postprocess.neighbourhood import neighbourhood_probabilities, fractions_skill_score, fss_from_sums
from efa_xray_amd.postprocess.pmmean import probability_matched_mean
from efa_xray_amd.postprocess.modes import (ensemble_gram, ensemble_eofs, ensemble_clusters, distances_from_gram,
                                            eofs_from_gram, clusters_from_gram)

__all__ = ["EnsembleState", "Observation", "gaspari_cohn", "haversine", "Assimilation", "EnSRF", "ETKF", "LETKF", "SlabLETKF", "ColumnInflation", "AdaptiveInflation",
           "observation_impact", "ensemble_sensitivity", "observation_targets",
           "ensemble_verification", "ensemble_products", "probability_verification",
           "ensemble_gram", "ensemble_eofs", "ensemble_clusters", "distances_from_gram", "eofs_from_gram", "clusters_from_gram",
           "neighbourhood_probabilities", "fractions_skill_score", "fss_from_sums",
           "probability_matched_mean", "sampling_error_table"]
__version__ = "0.1.0"
