"""Tracks as pose graphs: the layer between pairwise registration and Engine.pose_graph_optimize (multiway registration).

A tracker's crops give pairs of one object in two frames (tracklets.held_pairs); registering them gives a transform per pair, and
evaluate_registration an information matrix.  build_graphs turns the pairs of a track into one pose graph: a node per frame, an odometry edge per
pair of consecutive frames, a loop-closure edge (down-weighted by the line process when it disagrees with the rest) per pair further apart.  The
optimised poses are the object's frame at every time step, mapped into its frame at the track's first frame: a trajectory in which no single pairwise
error stays, where chaining the consecutive transforms keeps them all."""
from collections import OrderedDict

import numpy as np


def inverse(T):
    """The inverse of a rigid 4 x 4: (R^T, -(R^T t))."""
    T = np.asarray(T, np.float64).reshape(4, 4)
    out = np.eye(4)
    out[:3, :3] = T[:3, :3].T
    out[:3, 3] = -(T[:3, :3].T @ T[:3, 3])
    return out


def chain(odometry):
    """Poses [n, 4, 4] from the n - 1 transforms between consecutive frames (frame k into frame k + 1): X_0 = I, X_{k+1} = X_k T_{k,k+1}^-1."""
    X = [np.eye(4)]
    for T in odometry:
        X.append(X[-1] @ inverse(T))
    return np.stack(X)


def build_graphs(pairs, transforms, informations, centres, max_skip):
    """One pose graph per unbroken stretch of a track.  pairs: tracklets.HeldPair (or Pair) of gaps 1 .. max_skip, any order, any mix of sequences and
    tracks; transforms [B, 4, 4]: pair b's first crop into its second crop's frame; informations [B, 6, 6] and centres [B, 3]: Engine.evaluate_registration*
    (want_information=True, centers=centres) for those transforms, the centres in the second crop's frame.
    Pairs are grouped by (seq, track); a track is split where two of its frames are not joined by a gap-1 pair (a hole), a pair across a hole is
    dropped and so is a frame left on its own; pairs of a gap above max_skip are ignored.  Per stretch: a node per frame in frame order, a CERTAIN edge per gap-1 pair, an UNCERTAIN edge per
    pair of gap 2 .. max_skip, edges in the order of `pairs`, and initial poses chained from the gap-1 transforms (chain).
    Returns a list, ordered by (seq, track, first frame), of dict(seq, track, frames [n], timestamps [n] (None without them), pair_index [m] (which pair each
    edge is), and the graph: poses [n, 4, 4], i, j [m], T [m, 4, 4], info [m, 6, 6], c [m, 3], uncertain [m])."""
    if max_skip < 1:
        raise ValueError("max_skip = %r: expected >= 1" % (max_skip,))
    transforms = np.asarray(transforms, np.float64).reshape(-1, 4, 4)
    informations = np.asarray(informations, np.float64).reshape(-1, 6, 6)
    centres = np.asarray(centres, np.float64).reshape(-1, 3)
    if not (len(pairs) == len(transforms) == len(informations) == len(centres)):
        raise ValueError("build_graphs: %d pairs, %d transforms, %d informations, %d centres" % (len(pairs), len(transforms), len(informations), len(centres)))
    groups = OrderedDict()
    for b, p in enumerate(pairs):
        gap = int(p.frames[1]) - int(p.frames[0])
        if 1 <= gap <= max_skip:
            groups.setdefault((int(p.seq), int(p.track)), []).append(b)
    out = []
    for (seq, track), members in sorted(groups.items()):
        odo = {int(pairs[b].frames[0]): b for b in members if pairs[b].frames[1] - pairs[b].frames[0] == 1}
        frames = sorted({int(f) for b in members for f in pairs[b].frames})
        stamps = {}
        for b in members:
            for f, t in zip(pairs[b].frames, getattr(pairs[b], "timestamps", (None, None))):
                stamps[int(f)] = t
        stretch, stretches = [frames[0]], []
        for f in frames[1:]:
            if f - 1 == stretch[-1] and f - 1 in odo:
                stretch.append(f)
            else:
                stretches.append(stretch)
                stretch = [f]
        stretches.append(stretch)
        for fr in stretches:
            if len(fr) < 2:     # a frame that only pairs across holes reach: nothing joins it to anything
                continue
            node = {f: k for k, f in enumerate(fr)}
            used = [b for b in members if int(pairs[b].frames[0]) in node and int(pairs[b].frames[1]) in node]
            ts = [stamps[f] for f in fr]
            out.append(dict(seq=seq, track=track, frames=np.array(fr, np.int64), timestamps=None if any(t is None for t in ts) else np.array(ts, np.float64),
                            pair_index=np.array(used, np.int64), poses=chain([transforms[odo[f]] for f in fr[:-1]]),
                            i=np.array([node[int(pairs[b].frames[0])] for b in used], np.int32), j=np.array([node[int(pairs[b].frames[1])] for b in used], np.int32),
                            T=transforms[used].copy(), info=informations[used].copy(), c=centres[used].copy(),
                            uncertain=np.array([pairs[b].frames[1] - pairs[b].frames[0] > 1 for b in used], bool)))
    return out


def positions(poses, anchor):
    """Where the object is in every frame [n, 3]: X_k^-1 anchor, anchor = a point of the object in the first frame (its crop's mean).  A pose maps frame
    k onto frame 0, so its inverse carries the first frame's object to where frame k's crop has it."""
    anchor = np.asarray(anchor, np.float64).reshape(3)
    return np.stack([inverse(X)[:3, :3] @ anchor + inverse(X)[:3, 3] for X in np.asarray(poses, np.float64).reshape(-1, 4, 4)])


def speeds(poses, timestamps, anchor):
    """The xy speed between consecutive poses [n, 4, 4] over the timestamps [n]: n - 1 values, the xy distance between consecutive positions(poses, anchor)
    over the time between the frames."""
    d = np.diff(positions(poses, anchor)[:, :2], axis=0)
    return np.sqrt((d * d).sum(1)) / np.diff(np.asarray(timestamps, np.float64).ravel())
