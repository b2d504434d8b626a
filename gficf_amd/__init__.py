"""gficf_amd — MI355X (gfx950) GF-ICF normalisation and Phenograph kNN -> Jaccard edge build.

Drop-in for one hot path of the dibbelab/gficf R package: ``gficf()`` (sparse GF / ICF /
L2 scaling of a CSC genes x cells matrix) and the Jaccard step of ``clustcells()``
(``rcpp_parallel_jaccard_coef``), plus the exact neighbour search in front of it (``find_nn``).  All compute runs in hand-written HIP kernels behind the C
ABI of ``libgficf_hip.so`` (include/gficf_hip.h); there is no CPU fallback.
"""
from ._lib import GficfError, LIB_PATH  # noqa: F401
from .api import (  # noqa: F401
    Context,
    MultiContext,
    cluster_markers,
    cluster_signatures,
    clustcells,
    classify_cells,
    clustcells_graph,
    computePCADim,
    csc_tmm,
    find_ab_params,
    find_nn,
    find_nn_query,
    fuzzy_simplicial_set,
    HipOps,
    default_context,
    embedNewCells,
    device_count,
    fgsea,
    findClusterMarkers,
    gficf,
    gficf_with_weights,
    gmt_pathways,
    gsea,
    jaccard_adjacency,
    jaccard_coeff,
    jaccard_counts,
    jaccard_edges,
    jaccard_expand,
    knn_classify,
    phenograph,
    p_adjust_fdr,
    pca_dim_rule,
    pca_project,
    rcpp_parallel_jaccard_coef,
    rcpp_parallel_WMU_test,
    rcpp_WMU_test,
    rsvd,
    runGSEA,
    runLSA,
    runPCA,
    runReduction,
    run_modularity_clustering,
    transpose_gficf,
    umap,
    umap_init,
    umap_layout,
    umap_transform,
)

__version__ = "0.2.0"
