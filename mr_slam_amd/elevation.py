"""Elevation mapping over the C ABI (row N3): host-side mirror of the reference's libgpu.so functions
(Mapping/src/elevation_mapping_periodical/elevation_mapping/cuda/gpu_process.cu:938-1312)."""
import numpy as np

from . import _lib


def _f(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _i(a):
    return np.ascontiguousarray(a, dtype=np.int32)


class ElevationMap(_lib.Handle):
    _destroy = "mrs_elev_destroy"

    def __init__(self, length, resolution, mahalanobis_threshold=2.0, obstacle_threshold=0.6, device=0):
        self.L = int(length)
        self._create("mrs_elev_create", _lib.ctx(device), self.L, resolution, mahalanobis_threshold, obstacle_threshold)

    def move(self, position3):
        p = _f(position3); c = np.zeros(2, np.float32); s = np.zeros(2, np.int32); a = np.zeros(2, np.float32)
        _lib.load().mrs_elev_move(self._h, p, c, s, a)
        return c, s, a

    def process_points(self, x, y, z, transform, lower, upper, min_r, beam_a, beam_c, sensor_jacobian, rotation_variance,
                       c_sb_transpose, p_mul_c_bm_transpose, b_r_bs_skew):
        x, y, z = _f(x).copy(), _f(y).copy(), _f(z).copy()
        n = x.size
        mi = np.empty(n, np.int32)
        var, xt, yt, zt = (np.empty(n, np.float32) for _ in range(4))
        T = _f(transform).reshape(16)
        _lib.load().mrs_elev_process_points(self._h, n, x, y, z, T, lower, upper, min_r, beam_a, beam_c, _f(sensor_jacobian).reshape(3),
                                            _f(rotation_variance).reshape(9), _f(c_sb_transpose).reshape(9),
                                            _f(p_mul_c_bm_transpose).reshape(3), _f(b_r_bs_skew).reshape(9), mi, var, xt, yt, zt)
        return dict(map_index=mi, x=x, y=y, z=z, var=var, x_ts=xt, y_ts=yt, z_ts=zt)

    def fuse(self, index, color_r, color_g, color_b, intensity, height, var):
        arrs = [_i(index), _i(color_r), _i(color_g), _i(color_b), _f(intensity), _f(height), _f(var)]
        _lib.load().mrs_elev_fuse(self._h, arrs[0].size, *arrs)

    def mapvar_update(self, v):
        _lib.load().mrs_elev_mapvar_update(self._h, v)

    def map_feature(self):
        n = self.L * self.L
        f = {k: np.empty(n, np.float32) for k in ("elevation", "var", "rough", "slope", "traver", "intensity")}
        c = {k: np.empty(n, np.int32) for k in ("colorR", "colorG", "colorB")}
        _lib.load().mrs_elev_map_feature(self._h, f["elevation"], f["var"], c["colorR"], c["colorG"], c["colorB"], f["rough"], f["slope"],
                                         f["traver"], f["intensity"])
        f.update(c)
        return f

    def raytracing(self):
        _lib.load().mrs_elev_raytracing(self._h)

    def map_optmove(self, opt_p, height_update):
        a = np.zeros(2, np.float32)
        _lib.load().mrs_elev_map_optmove(self._h, _f(opt_p), height_update, a)
        return a

    def map_closeloop(self, update_position, height_update):
        _lib.load().mrs_elev_map_closeloop(self._h, _f(update_position), height_update)

    def layer(self, which):
        out = np.empty(self.L * self.L, np.float32)
        _lib.load().mrs_elev_get_layer(self._h, int(which), out)
        return out

    def frame(self):
        c = np.zeros(2, np.float32); s = np.zeros(2, np.int32)
        _lib.load().mrs_elev_get_frame(self._h, c, s)
        return c, s
