"""Utilities of the path: the reference's ``flashdeconv/utils`` re-exports (utils/__init__.py:3-31), the evaluation metrics
(``compute_rmse`` / ``compute_correlation``, utils/metrics.py) among them; the rest of the metrics are in ``utils.metrics``;
``spatial_autocorrelation`` / ``spatial_permutation_test`` (``utils.spatial_stats``), ``local_spatial_statistics`` (``utils.local_stats``), ``spatial_correlogram`` (``utils.correlogram``) and ``spatial_niches`` / ``kmeans`` / ``kmeans_plusplus`` (``utils.niches``) and
``celltype_expression`` / ``weighted_gene_sums`` / ``nnls_gram`` (``utils.expression``) and ``spatially_variable_genes`` /
``gene_spatial_sums`` / ``assemble_genes`` (``utils.spatial_genes``) and ``spatial_gene_pairs`` / ``gene_pair_sums`` /
``assemble_pairs`` (``utils.gene_pairs``) and ``spatial_gene_modules`` / ``spatial_coexpression`` / ``gene_coexpression_sums`` /
``assemble_coexpression`` (``utils.gene_modules``) and ``spatial_gene_permutation_test`` / ``gene_permutation_sums`` /
``assemble_gene_permutation`` (``utils.gene_permutations``) and ``rank_genes_groups`` / ``gene_group_sums`` / ``assemble_group_tests``
(``utils.group_genes``) and ``neighborhood_enrichment`` / ``label_pair_counts`` / ``join_count_moments`` / ``assemble_enrichment``
(``utils.neighborhoods``) and ``label_cooccurrence`` / ``label_band_counts`` / ``assemble_cooccurrence`` (``utils.cooccurrence``) and
``ligand_receptor_test`` / ``label_gene_sums`` / ``assemble_ligrec`` (``utils.ligrec``) are additive."""
from .genes import select_hvg, select_markers, compute_leverage_scores  # noqa: F401
from .graph import build_knn_graph, build_radius_graph, coords_to_adjacency  # noqa: F401
from .random import check_random_state  # noqa: F401
from .metrics import compute_rmse, compute_correlation  # noqa: F401
from .spatial_stats import spatial_autocorrelation, spatial_permutation_test, permutation_indices, randomization_variance  # noqa: F401
from .local_stats import local_spatial_statistics, conditional_indices  # noqa: F401
from .correlogram import spatial_correlogram  # noqa: F401
from .niches import spatial_niches, kmeans, kmeans_plusplus  # noqa: F401
from .expression import celltype_expression, weighted_gene_sums, nnls_gram  # noqa: F401
from .spatial_genes import spatially_variable_genes, gene_spatial_sums, assemble_genes  # noqa: F401
from .gene_pairs import spatial_gene_pairs, gene_pair_sums, assemble_pairs  # noqa: F401
from .gene_modules import spatial_gene_modules, spatial_coexpression, gene_coexpression_sums, assemble_coexpression  # noqa: F401
from .gene_permutations import spatial_gene_permutation_test, gene_permutation_sums, assemble_gene_permutation  # noqa: F401
from .group_genes import rank_genes_groups, gene_group_sums, assemble_group_tests  # noqa: F401
from .neighborhoods import neighborhood_enrichment, label_pair_counts, join_count_moments, assemble_enrichment  # noqa: F401
from .cooccurrence import label_cooccurrence, label_band_counts, assemble_cooccurrence  # noqa: F401
from .ligrec import ligand_receptor_test, label_gene_sums, assemble_ligrec  # noqa: F401

__all__ = ["select_hvg", "select_markers", "compute_leverage_scores", "build_knn_graph", "build_radius_graph",
           "coords_to_adjacency", "check_random_state", "compute_rmse", "compute_correlation",
           "spatial_autocorrelation", "spatial_niches", "kmeans", "kmeans_plusplus", "spatial_permutation_test",
           "permutation_indices", "randomization_variance", "local_spatial_statistics", "conditional_indices",
           "spatial_correlogram", "celltype_expression", "weighted_gene_sums", "nnls_gram", "spatially_variable_genes",
           "gene_spatial_sums", "assemble_genes", "rank_genes_groups", "gene_group_sums", "assemble_group_tests",
           "spatial_gene_permutation_test", "gene_permutation_sums", "assemble_gene_permutation",
           "neighborhood_enrichment", "label_pair_counts", "join_count_moments", "assemble_enrichment",
           "label_cooccurrence", "label_band_counts", "assemble_cooccurrence",
           "ligand_receptor_test", "label_gene_sums", "assemble_ligrec",
           "spatial_gene_pairs", "gene_pair_sums", "assemble_pairs",
           "spatial_gene_modules", "spatial_coexpression", "gene_coexpression_sums", "assemble_coexpression"]
