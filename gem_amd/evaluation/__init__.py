from gem_amd.evaluation.reconstruction import (evaluateStaticGraphReconstruction, evaluate_reconstruction_gpu, pair_metrics,  # noqa: F401
                                               random_edge_pairs, sampled_ap_gpu)
from gem_amd.evaluation.link_prediction import (evaluateStaticLinkPrediction, evaluate_link_prediction_gpu, link_prediction_dense,  # noqa: F401
                                                link_prediction_rows)
from gem_amd.evaluation.clustering import KMeans, clustering_scores, evaluateClustering, expClustering  # noqa: F401
from gem_amd.evaluation.ranking import argsort_desc, binary_ranking_scores, precision_recall_curve, roc_curve  # noqa: F401
from gem_amd.evaluation.link_classification import (EdgeClassifier, evaluateStaticLinkClassification, evaluate_link_classification,  # noqa: F401
                                                    expLinkClassification, sample_non_edges)
from gem_amd.evaluation.node_classification import (NodeClassifier, evaluateNodeClassification, expNC, f1_from_counts, label_csr,  # noqa: F401
                                                    split_nodes)
