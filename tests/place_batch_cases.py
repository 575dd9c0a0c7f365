"""Per-camera id lists for the batched place candidates' tests (include/svo.h, "Batched place candidates"), over the vote scenes of
tests/place_cases.py; shared by the host program's vectors and the GPU tests.  Every list is built once and never changed."""
import functools

import numpy as np

import place_cases as pc

SLICES = (0, 1, 63, 64, 65, 4096)                     # the entries of the six cameras of mixed_lists
HELD_BY = (1, 2, 64, 65, 66)                          # in how many of shared_lists' 66 cameras each planted id is


def _frozen(lists):
    for a in lists:
        a.setflags(write=False)
    return tuple(lists)


@functools.lru_cache(maxsize=None)
def mixed_lists(kind):
    """six cameras of 0, 1, 63, 64, 65 and 4096 ids: place_cases.id_list's — duplicates inside a list, ids absent from the index, ids
    0 and 2^64 - 1, colliding ids — and, since they are drawn from one universe, ids that several cameras hold"""
    return _frozen([np.array(pc.id_list(kind, n)) for n in SLICES])


@functools.lru_cache(maxsize=None)
def shared_lists(kind):
    """66 cameras of 8 ids: five planted ids in use, held by 1, 2, 64, 65 and all 66 cameras (the first ones), id 0 in every second
    camera, 2^64 - 1 in every third, the rest the camera's own draw from the ids in use"""
    rng = np.random.default_rng(4100)
    u = pc.vote_scene(kind)["universe"]
    lists = []
    for b in range(66):
        own = list(u[rng.integers(20, len(u), 8)])
        plant = [u[10 + i] for i, k in enumerate(HELD_BY) if b < k] + ([u[0]] if b % 2 == 0 else []) + ([u[1]] if b % 3 == 0 else [])
        lists.append(np.array((plant + own)[:8], np.uint64))
    return _frozen(lists)


@functools.lru_cache(maxsize=None)
def colliding_lists(kind, cameras=5, per_camera=8):
    """cameras x per_camera ids whose probes all start at ONE slot of the table over cameras * per_camera entries (fuse_cases'
    construction): up to six distinct ids in use, every camera holding each of them, some twice"""
    u = pc.vote_scene(kind)["universe"]
    clash = pc.colliding(u, cameras * per_camera, 6)
    lists = [np.array([clash[(b + i) % len(clash)] for i in range(per_camera)], np.uint64) for b in range(cameras)]
    return _frozen(lists)


@functools.lru_cache(maxsize=None)
def small_lists(kind, cameras, per_camera=4):
    """cameras x per_camera ids drawn from the ids in use: neighbours share ids"""
    rng = np.random.default_rng(4200 + cameras)
    u = pc.vote_scene(kind)["universe"]
    pool = u[rng.integers(0, len(u), 64)]
    return _frozen([np.array(pool[rng.integers(0, 64, per_camera)]) for _ in range(cameras)])


def offsets(lists):
    begin = np.zeros(len(lists) + 1, np.int32)
    begin[1:] = np.cumsum([len(a) for a in lists])
    return begin
