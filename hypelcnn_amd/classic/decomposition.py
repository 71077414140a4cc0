"""Band PCA for the classic-ML baselines: sklearn.decomposition.PCA over the band axis of a scene that is resident on the
device as float32 pixels, fitted by two streaming launches (hypel_pca_band_sums_f64, hypel_pca_scatter_f64) and applied
by one (hypel_pca_project_f32); include/hypel.h, csrc/pca.hip.

The eigen-decomposition of the covariance -- at most 512 x 512 -- is numpy.linalg.eigh in float64 on the host: a launch
would add nothing.  What the launches leave to the host is written out in `BandPCA.fit`: the float32 mean
the scatter is centred on differs from the float64 mean by d, and cov = S / (n - 1) - n / (n - 1) d d^T takes that back.

Not here: inverse_transform, incremental and randomised solvers, MNF, several scenes at once (GULFPORTALT)."""
import numbers

import numpy as np
import torch

from hypelcnn_amd.backend import PCA_CHUNK, PCA_MAX_BANDS, PCA_MAX_BLOCKS, PCA_TILE, Ref


def band_sums_ws_doubles(n, c):
    """doubles of workspace hypel_pca_band_sums_f64 asks for (include/hypel.h)"""
    return min(-(-n // PCA_CHUNK), PCA_MAX_BLOCKS) * c


def scatter_ws_doubles(n, c):
    """doubles of workspace hypel_pca_scatter_f64 asks for (include/hypel.h)"""
    nt = -(-c // PCA_TILE)
    tiles = nt * (nt + 1) // 2
    return min(-(-n // PCA_CHUNK), PCA_MAX_BLOCKS // tiles) * tiles * PCA_TILE * PCA_TILE


class ProjectedScene:
    """What `BandPCA.transform_scene` returns: the data set common_nn_ops.SceneArrays.feed and the estimators read, with
    the padded HSI raster replaced by its projection ([hp, wp, k]) and the LiDAR raster untouched."""

    def __init__(self, data_set, casi_dev, lidar_dev):
        self.casi_dev, self.lidar_dev = casi_dev, lidar_dev
        self.neighborhood = int(data_set.neighborhood)
        self.casi_scale = int(getattr(data_set, "casi_scale", 1))
        self._scene_shape = [int(v) for v in data_set.get_scene_shape()]

    def get_data_shape(self):
        side = self.neighborhood * 2 + 1
        lidar = 0 if self.lidar_dev is None else int(self.lidar_dev.shape[2])
        return [side, side, int(self.casi_dev.shape[2]) + lidar]

    def get_casi_band_count(self):
        return int(self.casi_dev.shape[2])

    def get_scene_shape(self):
        return list(self._scene_shape)


class BandPCA:
    """The subset of sklearn.decomposition.PCA (svd_solver="full") a band reduction needs.  n_components: an integer
    1..C, or a float in (0, 1) -- the smallest k whose cumulative explained-variance ratio exceeds it, scikit-learn's
    rule.  Fitted attributes: mean_ (float64 [C]), components_ (float64 [k, C]; the entry of largest magnitude of every
    component is positive, the first such entry on ties), explained_variance_ (ddof 1), explained_variance_ratio_,
    n_components_, n_samples_, n_features_in_."""

    def __init__(self, n_components, whiten=False, backend=None):
        self.n_components, self.whiten = n_components, bool(whiten)
        self._be = backend
        self.components_ = None
        nc = n_components
        if isinstance(nc, bool) or not isinstance(nc, numbers.Real) or not (
                (isinstance(nc, numbers.Integral) and nc >= 1) or (not isinstance(nc, numbers.Integral) and 0.0 < nc < 1.0)):
            raise ValueError(f"BandPCA: n_components={nc!r}: an integer >= 1 or a float in (0, 1)")

    def get_params(self):
        return {"n_components": self.n_components, "whiten": self.whiten}

    def _backend(self):
        if self._be is None:
            from hypelcnn_amd.backend import HipBackend
            self._be = HipBackend()
        return self._be

    def _view(self, pixels, tail=0, what="fit"):
        """[rows, C + tail] or [h, w, C + tail] (NumPy array: uploaded; device tensor: read in place through its strides)
        -> (flat tensor at the view's origin, h, w, C, stride_y, stride_x)"""
        be = self._backend()
        if isinstance(pixels, np.ndarray):
            t = torch.from_numpy(np.ascontiguousarray(pixels, dtype=np.float32)).to(be.device)
        else:
            t = pixels.to(be.device)
        if t.dtype != torch.float32:
            t = t.float()
        if t.dim() not in (2, 3) or t.shape[-1] - tail < 1 or min(t.shape) < 1:
            raise ValueError(f"BandPCA.{what}: pixels as [rows, bands] or [h, w, bands], got {tuple(t.shape)}")
        if t.dim() == 2:
            t = t.unsqueeze(0)
        c = int(t.shape[2]) - tail
        if c > PCA_MAX_BANDS:
            raise ValueError(f"BandPCA.{what}: {c} bands; at most {PCA_MAX_BANDS} (HYPEL_PCA_MAX_BANDS)")
        h, w = int(t.shape[0]), int(t.shape[1])
        if (t.shape[2] > 1 and t.stride(2) != 1) or (w > 1 and t.stride(1) < c + tail) or (h > 1 and t.stride(0) < c + tail):
            t = t.contiguous()
        sx = int(t.stride(1)) if w > 1 else c + tail
        sy = int(t.stride(0)) if h > 1 else max(w * sx, c + tail)
        span = (h - 1) * sy + (w - 1) * sx + c + tail
        return t.as_strided((span,), (1,)), h, w, c, sy, sx

    def fit(self, view):
        """view: the pixels, [rows, C] or [h, w, C], a NumPy array or a (possibly strided) float32 device tensor."""
        be = self._backend()
        flat, h, w, c, sy, sx = self._view(view)
        n = h * w
        if n < 2:
            raise ValueError(f"BandPCA.fit: {n} pixel(s); a covariance needs at least 2")
        if isinstance(self.n_components, numbers.Integral) and self.n_components > c:
            raise ValueError(f"BandPCA.fit: n_components={self.n_components} of {c} bands")
        sums = be.zeros(c, torch.float64)
        need = band_sums_ws_doubles(n, c)
        be.call("pca_band_sums_f64", Ref(flat), h, w, c, sy, sx, Ref(sums), Ref(be.empty(need, torch.float64)), need)
        mean64 = sums.cpu().numpy().astype(np.float64) / n
        mean32 = mean64.astype(np.float32)
        scatter = be.zeros(c * c, torch.float64)
        need = scatter_ws_doubles(n, c)
        be.call("pca_scatter_f64", Ref(flat), h, w, c, sy, sx, Ref(be.upload(mean32)), Ref(scatter),
                Ref(be.empty(need, torch.float64)), need)
        s = scatter.cpu().numpy().astype(np.float64).reshape(c, c)
        # the scatter is centred on the float32 mean: sum (x - m32)(x - m32)^T = sum (x - m)(x - m)^T + n d d^T
        d = mean64 - mean32.astype(np.float64)
        cov = s / (n - 1) - (n / (n - 1)) * np.outer(d, d)
        values, vectors = np.linalg.eigh(cov)
        order = np.argsort(-values, kind="stable")
        values, vectors = np.clip(values[order], 0.0, None), vectors[:, order].T
        lead = np.argmax(np.abs(vectors), axis=1)  # (the first of equal magnitudes)
        vectors = vectors * np.where(vectors[np.arange(c), lead] < 0, -1.0, 1.0)[:, None]
        total = values.sum()
        ratio = values / total if total > 0 else np.zeros_like(values)
        if isinstance(self.n_components, numbers.Integral):
            k = int(self.n_components)
        else:
            k = min(c, int(np.searchsorted(np.cumsum(ratio), self.n_components, side="right")) + 1)
        if self.whiten and np.any(values[:k] <= 0):
            raise ValueError(f"BandPCA(whiten=True): component {int(np.argmax(values[:k] <= 0))} of the {k} kept has zero "
                             f"variance and cannot be scaled to unit variance")
        self.mean_, self.components_ = mean64, np.ascontiguousarray(vectors[:k])
        self.explained_variance_, self.explained_variance_ratio_ = values[:k].copy(), ratio[:k].copy()
        self.n_components_, self.n_samples_, self.n_features_in_ = k, n, c
        weights = self.components_.T  # [C, k]
        if self.whiten:
            weights = weights / np.sqrt(self.explained_variance_)[None, :]
        self._mean_d = be.upload(mean32)
        self._weights_d = be.upload(np.ascontiguousarray(weights, dtype=np.float32))
        return self

    @staticmethod
    def _single_scene(data_set, what):
        if getattr(data_set, "_data_sets", None) is not None:
            raise NotImplementedError(f"BandPCA.{what}: a MultiDataSet (GULFPORTALT) draws every sample from one of several "
                                      f"scenes; one band PCA over several scenes is not built (DESIGN 7)")

    def _resident(self, data_set):
        from hypelcnn_amd.common.common_nn_ops import SceneArrays
        return SceneArrays._resident(data_set, self._backend().device)

    def fit_scene(self, data_set):
        """Fits on the interior of the data set's padded HSI raster: the padding pixels are reflections of interior
        ones and are not counted."""
        self._single_scene(data_set, "fit_scene")
        casi, _ = self._resident(data_set)
        nb = int(data_set.neighborhood)
        hp, wp = int(casi.shape[0]), int(casi.shape[1])
        return self.fit(casi[nb:hp - nb, nb:wp - nb, :])

    def _fitted(self, what):
        if self.components_ is None:
            raise ValueError(f"BandPCA.{what}: fit first")

    def _project(self, flat, h, w, c, sy, sx, pass_cols, what):
        if c != self.n_features_in_:
            raise ValueError(f"BandPCA.{what}: pixels of {c} bands, the model was fitted on {self.n_features_in_}")
        be = self._backend()
        k = self.n_components_
        out = be.empty(h * w * (k + pass_cols))
        be.call("pca_project_f32", Ref(flat), h, w, c, sy, sx, pass_cols, Ref(self._mean_d), Ref(self._weights_d), k,
                Ref(out), k + pass_cols)
        return out

    def transform(self, rows, pass_cols=0):
        """rows: [n, C + pass_cols] -> [n, k + pass_cols]: the projection of the first C columns, the others copied
        through.  A NumPy array comes back as one, a device tensor as one."""
        self._fitted("transform")
        pass_cols = int(pass_cols)
        if pass_cols < 0 or getattr(rows, "ndim", 0) != 2:
            raise ValueError(f"BandPCA.transform: rows as [n, bands + pass_cols] with pass_cols >= 0, got "
                             f"{tuple(getattr(rows, 'shape', ()))} and pass_cols={pass_cols}")
        n = int(rows.shape[0])
        if n == 0:
            empty = np.zeros((0, self.n_components_ + pass_cols), np.float32)
            return empty if isinstance(rows, np.ndarray) else torch.from_numpy(empty).to(self._backend().device)
        flat, h, w, c, sy, sx = self._view(rows, pass_cols, "transform")
        out = self._project(flat, h, w, c, sy, sx, pass_cols, "transform").view(n, self.n_components_ + pass_cols)
        return out.cpu().numpy() if isinstance(rows, np.ndarray) else out

    def transform_scene(self, data_set):
        """The whole padded raster, padding included: the projection of a reflection is the reflection of the projection
        (a pixel gives the same bits wherever it lies).  -> ProjectedScene"""
        self._fitted("transform_scene")
        self._single_scene(data_set, "transform_scene")
        casi, lidar = self._resident(data_set)
        hp, wp = int(casi.shape[0]), int(casi.shape[1])
        flat, h, w, c, sy, sx = self._view(casi, 0, "transform_scene")
        out = self._project(flat, h, w, c, sy, sx, 0, "transform_scene")
        return ProjectedScene(data_set, out.view(hp, wp, self.n_components_), lidar)
