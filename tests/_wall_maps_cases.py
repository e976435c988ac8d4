"""Synthetic recordings for tests/test_wall_maps_host.py: synth_crowd_frames -> obsmat.txt -> create_dataset, and the map such a
test gives a recording (the bounding box of its true futures).  Nothing here touches the device."""
import numpy as np


def recording(tmp, seed, n_frames=60, n_ped=24, one_scene=False):
    """(obsvs, preds, batches, times) of one synthetic recording in world coordinates, shifted by 30 * seed so that the
    recordings do not overlap; one_scene: its largest scene alone."""
    from socialways_amd import data as D
    path = str(tmp / ("obsmat_%d.txt" % seed))
    fr, ids, pos, vel = D.synth_crowd_frames(n_frames=n_frames, n_ped=n_ped, seed=seed)
    D.write_biwi_obsmat(path, fr, ids, pos + 30.0 * seed, vel)
    p_data, t_data, interval = D.parse_biwi(path)
    o, p, t, b = D.create_dataset(p_data, t_data, range(int(t_data[0][0]), int(t_data[-1][-1]), interval))
    if one_scene:
        lo, hi = b[int(np.argmax(b[:, 1] - b[:, 0]))]
        return o[lo:hi], p[lo:hi], np.array([[0, hi - lo]], np.int64), list(t[lo:hi])
    return o, p, b, t


def box_walls(pts):
    """The four sides of the bounding box of points (.., 2) -> (4, 4) float32: x0 y0 x1 y1."""
    pts = np.asarray(pts, np.float64).reshape(-1, 2)
    lo, hi = pts.min(0), pts.max(0)
    return np.array([[lo[0], lo[1], hi[0], lo[1]], [hi[0], lo[1], hi[0], hi[1]], [hi[0], hi[1], lo[0], hi[1]],
                     [lo[0], hi[1], lo[0], lo[1]]], np.float32)
