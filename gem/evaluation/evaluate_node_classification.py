from gem_amd.evaluation.node_classification import evaluateNodeClassification, expNC  # noqa: F401
