from gem_amd.evaluation.reconstruction import (evaluateStaticGraphReconstruction, evaluate_reconstruction_gpu, pair_metrics,  # noqa: F401
                                               random_edge_pairs, sampled_ap_gpu)
