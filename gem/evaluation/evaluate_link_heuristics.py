from gem_amd.evaluation.link_heuristics import evaluateStaticLinkHeuristics, evaluate_link_heuristics, expLinkHeuristics  # noqa: F401
