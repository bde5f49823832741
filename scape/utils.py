"""``scape.utils`` import path of the reference's two reporting commands (utils.py:319-427, :438-553) and of
``ex_pa_pseudobulk``, which sums their count matrix over cell groups, and ``diff_pa`` / ``diff_pa_len``, which test
it between two (per pA site, and per gene for a shift of the 3'UTR length), and ``diff_pa_groups`` /
``diff_pa_len_groups``, which test the same two questions across all clusters at once, and ``diff_pa_pairs`` and
``diff_pa_markers``, which run ``diff_pa`` on every pair of clusters and on every cluster against all other cells,
``diff_pa_len_pairs`` and ``diff_pa_len_markers``, which run ``diff_pa_len`` on the same pairs and markers, and
``diff_pa_trend`` and ``diff_pa_len_trend``, which test pA usage and 3'UTR length along a per-cell score such as
pseudotime, and ``ex_pa_len_mat``, the gene x cell matrix of the expected pA length, and ``ex_pa_usage_mat``, the
pA site x cell matrix of the per-cell site usage, and ``boot_pa_len``, the
bootstrap intervals of a cluster's mean pA position and expected pA length, and ``boot_pa_usage``, those of its usage
of every pA site, and ``boot_pa_len_diff`` and ``boot_pa_usage_diff``, those of the difference of either between two
cell populations."""
from scape_amd.report import (boot_pa_len, boot_pa_len_diff, boot_pa_usage, boot_pa_usage_diff,  # noqa: F401
                              cal_exp_pa_len, diff_pa, diff_pa_groups,
                              diff_pa_len, diff_pa_len_groups, diff_pa_len_markers, diff_pa_len_pairs,
                              diff_pa_len_trend, diff_pa_markers, diff_pa_pairs, diff_pa_trend, ex_pa_cnt_mat,
                              ex_pa_len_mat, ex_pa_pseudobulk, ex_pa_usage_mat)
