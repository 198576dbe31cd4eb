from efa_xray_amd.postprocess.impact import observation_impact

__all__ = ["observation_impact"]
