"""The batched relocalisation beside frames in flight on a real GPU (include/svo.h, "Batched relocalisation"), after
tests/test_gpu_reloc_frames.py: a context of nine 320 x 160 sequences — a many-sequence context, as the batch's own stage context of
nine cameras is — with three frames in flight, and svo_desc_index_localize_batch called between submit and collect, guided and
unguided.  The call waits for the index's own stream only and its stage context takes no part in the device's LK gate: poses,
observation rows and descriptor rows of every sequence are bit for bit those of a run without it."""
import numpy as np
import pytest

import reloc_batch_cases as bc
from gpu_kit import api, projections, streams  # noqa: F401  (the fixture is found by name)

pytestmark = pytest.mark.gpu

W, H, N_SEQ, N_FRAMES, SEED0, ROWS = 320, 160, 9, 6, 900, 150
OVER = dict(max_translation_norm=2.0, ransac_reprojection_error=0.25)


def run_in_flight(api, with_index):
    """six frames of nine sequences as device frames, three in flight -> per frame (ok, poses, observation rows, descriptor rows) as bytes"""
    import torch
    seqs = streams(N_SEQ, N_FRAMES, SEED0, W, H)
    dev = [[(torch.from_numpy(L[k]).cuda(), torch.from_numpy(R[k]).cuda()) for L, R in seqs] for k in range(N_FRAMES)]
    torch.cuda.synchronize()
    vo = api.BatchVisualOdometry(W, H, N_SEQ, api.default_config(**OVER))
    vo.initalize_projection_matricies(*projections(W, H))
    vo.set_track_output(ROWS)
    vo.set_descriptor_output(True)
    ix = api.DescriptorIndex(4096, points=True) if with_index else None
    names, K, guides, queries, xys = bc.small(N_SEQ)
    out, located = [], 0
    try:
        if ix:
            bc.fill(ix, bc.index_rows())
        for k0 in range(0, N_FRAMES, 3):
            for k in range(k0, k0 + 3):
                vo.submit_device([a.data_ptr() for a, _ in dev[k]], [b.data_ptr() for _, b in dev[k]], W)
                if ix:                                                   # frames in flight: the call waits for its own stream only
                    located += sum(r.success for r, _ in ix.localize_batch(K, queries, xys, guides if k % 2 == 0 else None))
            for k in range(k0, k0 + 3):
                ok, T = vo.collect()
                out.append((ok.tobytes(), T.tobytes(), b"".join(vo.last_track_obs(i).tobytes() for i in range(N_SEQ)),
                            b"".join(vo.last_track_descriptors(i).tobytes() for i in range(N_SEQ))))
        if ix:
            assert located >= 3 * 3                                      # the guided calls locate `repeated`, `six` and the planned slices
    finally:
        vo.close()
        if ix:
            ix.close()
        del dev
    return out


def test_a_batch_call_beside_frames_in_flight_changes_nothing(api):
    plain, beside = run_in_flight(api, False), run_in_flight(api, True)
    assert len(plain) == len(beside) == N_FRAMES
    for k, (a, b) in enumerate(zip(plain, beside)):
        assert a[0] == b[0] and a[1] == b[1], "frame %d: ok / pose" % k
        assert a[2] == b[2], "frame %d: observation rows" % k
        assert a[3] == b[3], "frame %d: descriptor rows" % k
    assert sum(len(a[3]) for a in plain) > N_SEQ * 32 * 300
    assert np.frombuffer(plain[-1][0], np.uint8).any()
