"""click group exposing ``infer_pa``, its consumer ``merge_pa`` and the stages after it, ``cal_exp_pa_len``,
``ex_pa_cnt_mat``, ``ex_pa_pseudobulk`` (the sums the reference's DEXSeq script starts from), ``diff_pa`` (a
permutation test of pA usage between two cell populations), ``diff_pa_len`` (the same test on the mean pA position:
3'UTR lengthening or shortening), ``diff_pa_groups`` (diff_pa's omnibus form across all clusters) and
``diff_pa_len_groups`` (diff_pa_len's), ``diff_pa_pairs`` (diff_pa for every pair of clusters, adjusted over all of
them), ``diff_pa_markers`` (diff_pa for every cluster against all other cells), ``diff_pa_len_pairs`` and
``diff_pa_len_markers`` (diff_pa_len for the same pairs and markers), ``diff_pa_trend`` (pA usage along a
per-cell score such as pseudotime), ``diff_pa_len_trend`` (3'UTR length along the same score), ``boot_pa_len``
(bootstrap intervals of every cluster's mean pA position and expected pA length, by resampling the cells),
``boot_pa_usage`` (the same intervals of every cluster's usage of every pA site), ``boot_pa_len_diff`` and
``boot_pa_usage_diff`` (the intervals of the difference of either between two cell populations),
``ex_pa_len_mat`` (the gene x cell matrix of the expected pA length) and ``ex_pa_usage_mat`` (the pA site x cell matrix
of the per-cell site usage; the sixteen are this build's own last steps;
reference cli.py:7-31 registers six commands; ``gen_utr_annotation`` and ``prepare_input`` are outside this build's
scope)."""
import click

from scape_amd.apa_core import infer_pa, infer_pa_all, prebin
from scape_amd.junction_handler import merge_pa
from scape_amd.report import (boot_pa_len, boot_pa_len_diff, boot_pa_usage, boot_pa_usage_diff, cal_exp_pa_len,
                              diff_pa, diff_pa_groups, diff_pa_len, diff_pa_len_groups, diff_pa_len_markers,
                              diff_pa_len_pairs, diff_pa_len_trend, diff_pa_markers, diff_pa_pairs, diff_pa_trend,
                              ex_pa_cnt_mat, ex_pa_len_mat, ex_pa_pseudobulk, ex_pa_usage_mat)


@click.group()
def cli():
    """SCAPE-APA `infer_pa` on AMD MI355X (HIP kernels behind the reference's CLI)."""


def display_paper_info():
    print()
    print("scape infer_pa (MI355X/HIP build). Method: SCAPE-APA, Cheng, Le, Zhou, Cheng,")
    print("bioRxiv 2024, https://doi.org/10.1101/2024.03.12.584547")
    print()


cli.add_command(infer_pa)
cli.add_command(infer_pa_all)
cli.add_command(merge_pa)
cli.add_command(prebin)
cli.add_command(cal_exp_pa_len)
cli.add_command(ex_pa_cnt_mat)
cli.add_command(ex_pa_len_mat)
cli.add_command(ex_pa_usage_mat)
cli.add_command(ex_pa_pseudobulk)
cli.add_command(diff_pa)
cli.add_command(diff_pa_len)
cli.add_command(diff_pa_groups)
cli.add_command(diff_pa_len_groups)
cli.add_command(diff_pa_pairs)
cli.add_command(diff_pa_markers)
cli.add_command(diff_pa_len_pairs)
cli.add_command(diff_pa_len_markers)
cli.add_command(diff_pa_trend)
cli.add_command(diff_pa_len_trend)
cli.add_command(boot_pa_len)
cli.add_command(boot_pa_usage)
cli.add_command(boot_pa_len_diff)
cli.add_command(boot_pa_usage_diff)
