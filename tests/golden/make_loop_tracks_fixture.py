"""Vendors the loop-track INPUT DATA the track stage is pinned on: kitti00/loop_tracks_29pairs.npy.

    python tests/golden/make_loop_tracks_fixture.py <the reference's data/map000000>

loopTracks.txt is data the reference's program wrote (computeConstraints, kittiDetector.h:1493-1501): a count, then one
line "2 frame keypoint frame keypoint" per kept match of every loop pair, the pairs one after the other.  The fixture
keeps the matches of the pairs that touch a frame occurring in more than one pair, as int16 [n, 4] = frame, keypoint,
frame, keypoint in file order: every track of length 3 and 4 that SaveAsSfMInit's connection loop
(kitti_surf.cpp:349-391) builds from the full file is in it.  No source is copied.

The script re-derives what tests/test_track_ref.py expects, with a serial restatement of that loop on the full file and
on the fixture, and prints it."""
import collections
import os
import sys

import numpy as np

DST = os.path.join(os.path.dirname(os.path.abspath(__file__)), "kitti00", "loop_tracks_29pairs.npy")


def connect(rows):
    """The loop of kitti_surf.cpp:349-391: (tracks by their key, matches dropped by the 'both already seen' rule)"""
    tracks, seen, dropped = {}, {}, 0
    for key, (f0, k0, f1, k1) in enumerate(rows):
        a, b = (f0, k0), (f1, k1)
        ta, tb = seen.get(a), seen.get(b)
        if ta is None and tb is None:
            tracks[key] = [a, b]
            seen[a] = seen[b] = key
        elif ta is None:
            seen[a] = tb
            tracks[tb].append(a)
        elif tb is None:
            seen[b] = ta
            tracks[ta].append(b)
        else:
            dropped += 1
    return tracks, dropped


def components(rows):
    """The plain connected components of the match graph, as a set of frozensets"""
    parent = {}

    def find(x):
        while parent.setdefault(x, x) != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for f0, k0, f1, k1 in rows:
        a, b = find((f0, k0)), find((f1, k1))
        if a != b:
            parent[max(a, b)] = min(a, b)
    out = collections.defaultdict(set)
    for x in list(parent):
        out[find(x)].add(x)
    return {frozenset(v) for v in out.values()}


def report(name, rows):
    tracks, dropped = connect(rows)
    lengths = collections.Counter(len(t) for t in tracks.values())
    twice = sum(len({f for f, _ in t}) != len(t) for t in tracks.values())
    same = {frozenset(t) for t in tracks.values()} == components(rows)
    print(f"{name}: {len(rows)} matches -> {len(tracks)} tracks, lengths {dict(sorted(lengths.items()))}, "
          f"{dropped} dropped, {twice} with a frame twice, equal to the connected components: {same}")


def main(src):
    with open(os.path.join(src, "loopTracks.txt")) as f:
        count = int(f.readline())
        rows = [tuple(int(x) for x in ln.split()[1:]) for ln in f if ln.strip()]
    assert len(rows) == count and all(len(r) == 4 for r in rows)
    pair_of = [(r[0], r[2]) for r in rows]
    pairs = [p for i, p in enumerate(pair_of) if i == 0 or p != pair_of[i - 1]]
    assert len(set(pairs)) == len(pairs), "the matches of a pair are consecutive"
    in_pairs = collections.Counter(f for p in pairs for f in set(p))
    recurring = {f for f, n in in_pairs.items() if n > 1}
    kept_pairs = [p for p in pairs if recurring & set(p)]
    keep = set(kept_pairs)
    kept = [r for r, p in zip(rows, pair_of) if p in keep]
    print(f"{len(pairs)} pairs over {len(in_pairs)} frames, {len(recurring)} frames in more than one pair, "
          f"{len(kept_pairs)} pairs touch one")
    report("full file", rows)
    report("fixture", kept)
    a = np.array(kept, dtype=np.int64)
    assert a.min() >= 0 and a.max() < 2 ** 15
    np.save(DST, a.astype(np.int16))
    print(DST, os.path.getsize(DST), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
