"""The item arrays of gmm_aligner_posteriors_device go, untouched and without leaving the device, into
Estimator.accumulate_posteriors_device: score -> Baum-Welch alignment -> accumulation.  The tables equal, bit for bit,
those of a second estimator that is fed the same list from host arrays."""
import numpy as np
import pytest

import rasr_amd as ra
from rasr_amd.aligner import batch_graphs, linear_hmm_graph

pytestmark = pytest.mark.gpu


def test_items_feed_the_estimator(gpu):
    import torch
    D, n_mix = 3, 6
    top = ra.synthetic_mixture_set(n_mix, [3, 1, 2, 3, 2, 1], D, seed=17, weights="random")
    frames = ra.synthetic_frames(23, D, seed=18)
    scorer = ra.Scorer(top, "diagonal-sum", max_frames=23)
    d_frames = torch.from_numpy(frames).to(gpu)
    d_scores = torch.empty((n_mix, 23), dtype=torch.float32, device=gpu)
    scorer.score_device(d_frames, d_scores)
    # two segments with a gap: columns 1..10 and 13..22
    graphs = [linear_hmm_graph([0, 3, 5, 2], 1.0, 0.5, 2.0, 0.25), linear_hmm_graph([4, 1, 0], 0.75, 0.5, 1.5, 0.0, repeat=2)]
    b = batch_graphs(graphs, [1, 13], [10, 10])
    aligner = ra.Aligner(2, int(b["state_offset"][-1]), int(b["arc_offset"][-1]), 10 * (5 + 7), n_mix)
    aligner.set_segments(**b)
    r = aligner.posteriors(d_scores, pruning_threshold=50.0)
    n = r["n_items"]
    assert n > 20 and (r["score"].cpu().numpy() < 1e30).all()
    weight = r["weight"].cpu().numpy()
    offset = r["column_offset"].cpu().numpy()
    assert offset[1] == 0 and offset[11] == offset[13] and offset[23] == n
    sums = np.add.reduceat(weight, offset[[*range(1, 11), *range(13, 23)]])
    assert np.abs(sums - 1.0).max() < 1e-5
    assert len(set(weight.tolist())) > 5, "soft weights, not a Viterbi path"

    device = ra.Estimator(top, max_pairs=3 * n)
    device.accumulate_posteriors_device(d_frames, r["frame"], r["mixture"], r["weight"], scorer=scorer)
    host = ra.Estimator(top, max_pairs=3 * n)
    host.accumulate_posteriors_host(frames, r["frame"].cpu().numpy().view(np.uint32),
                                    r["mixture"].cpu().numpy().view(np.uint32), weight, scorer=scorer)
    torch.cuda.synchronize()
    got, want = device.get(), host.get()
    assert got["entry_weights"].sum() > 0
    for k in want:
        assert np.array_equal(got[k].view(np.uint64), want[k].view(np.uint64)), k
