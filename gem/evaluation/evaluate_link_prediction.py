from gem_amd.evaluation.link_prediction import evaluateStaticLinkPrediction, evaluate_link_prediction_gpu  # noqa: F401
