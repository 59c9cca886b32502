#!/usr/bin/env python3
"""eval_depth_edges.py -- the reference's edge benchmark ("AUC (edges)", reference eval_depth_edges.py:377-416) on an MI355X.

Canny edges of every predicted depth map (.npy, metres) at the twelve thresholds 20 .. 240, a one-to-one correspondence of
predicted and annotated edge pixels (.png annotations, 1-bit or 8-bit) within 0.002 of the image diagonal, pooled precision and
recall per threshold, and the mean recall over the precision range -- all of it in mindtheedge_amd/utils/edge_benchmark.py.
Same six arguments and the same two printed lines as the reference.  ``--temp_save_path`` is accepted and unused: no edge image
is written to disk (the reference's JPEG round trip is left out on purpose)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    parser = argparse.ArgumentParser(description='Edge AUC benchmark of predicted depth maps on MI355X')
    parser.add_argument('--depth_pred_list_path', type=str,
                        help='List of predicted depth image *names* in .npy format (with metric depth)')
    parser.add_argument('--depth_pred_dir_path', type=str,
                        help='Path to the directory that contains the depth images (.npy files)')
    parser.add_argument('--depth_edge_gt_list_path', default='data/kitti_de/kitti_de_annotated_edges.txt', type=str,
                        help='List of GT depth edge image *names* in .png format')
    parser.add_argument('--depth_edge_gt_dir_path', default='data/kitti_de/gt', type=str,
                        help='Path to the directory that contains the depth edges GT (.png files)')
    parser.add_argument('--temp_save_path', default='temp_output', type=str, help='accepted for compatibility; nothing is written')
    parser.add_argument('--prec_recall_eval_range_min', default=0.12, type=float, help='Min range for edge AUC computation')
    parser.add_argument('--prec_recall_eval_range_max', default=0.65, type=float, help='Max range for edge AUC computation')
    args = parser.parse_args()
    from mindtheedge_amd.utils.edge_benchmark import evaluate_lists

    def paths(list_path, dir_path):
        with open(list_path) as f:
            return [dir_path + '/' + x.strip().split('/')[-1] for x in f.read().splitlines() if x.strip()]
    _, _, f1, f2 = evaluate_lists(paths(args.depth_pred_list_path, args.depth_pred_dir_path),
                                  paths(args.depth_edge_gt_list_path, args.depth_edge_gt_dir_path),
                                  args.prec_recall_eval_range_min, args.prec_recall_eval_range_max)
    print('AUC over all range: ' + str(f1) + '\n')
    print('AUC over partial range: ' + str(f2) + '\n')


if __name__ == '__main__':
    main()
