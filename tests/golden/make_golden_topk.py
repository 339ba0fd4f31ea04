"""Capture the reference's top-K centre parsing (authoring container only).

    python tests/golden/make_golden_topk.py

Runs the REAL reference's CenterMap.parse_centermap_heatmap_adaptive_scale_batch (imported through ref_shim.py) with
train_flag=True and max_hand = K on the seeded centre maps of tests/multi_ref.py and writes decode_topk.npz: per case and K
the reference's batch_ids, flat indices and scores.  The maps themselves are not stored: multi_ref.topk_case_maps rebuilds
them from their seeds.  torch.topk leaves the order of exact ties open, so the script refuses maps whose detections tie.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import multi_ref  # noqa: E402
import ref_shim  # noqa: E402


def main():
    ref_model, ref_parser, ref_wrapper, ref_manolayer, ref_utils = ref_shim.import_reference()
    centermap_parser = ref_parser.CenterMap()
    assert abs(centermap_parser.conf_thresh - multi_ref.CONF_THRESH) < 1e-12
    out = {}
    for name in multi_ref.TOPK_CASES:
        maps, counts = multi_ref.topk_case_maps(name)
        for m in maps:      # no exact tie among the detections (and the first loser) of a map
            det = np.sort(multi_ref.nms_det(m[0]).reshape(-1))[::-1][:multi_ref.MAX_HAND + 1]
            det = det[det > 0]
            assert len(np.unique(det)) == len(det), '%s: tied detections' % name
        for K in multi_ref.TOPK_KS:
            centermap_parser.max_hand = K
            with torch.no_grad():
                ids, inds, yxs, scores = centermap_parser.parse_centermap_heatmap_adaptive_scale_batch(torch.from_numpy(maps),
                                                                                                       train_flag=True)
            out['%s_k%d_batch_ids' % (name, K)] = ids.numpy().astype(np.int64)
            out['%s_k%d_inds' % (name, K)] = inds.numpy().astype(np.int64)
            out['%s_k%d_scores' % (name, K)] = scores.numpy().astype(np.float32)
            print(name, 'K', K, 'detections per frame', counts, '->', ids.numpy().tolist())
    path = os.path.join(HERE, 'decode_topk.npz')
    np.savez_compressed(path, **out)
    print('decode_topk.npz', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
