"""The float64 statement of the Dense backward (csrc/dense_grad.hip): y = relu?(x . w^T + b), x [rows, cin], w [cout, cin],
y / dy [rows, cout].  dz = dy where y_relu > 0 else 0 (TF ReluGrad: strict '>', a select -- a NaN in dy under a closed gate
gives 0); dx = dz . w, kept where x_relu > 0; dw = dz^T . x; db = the column sums of dz.  The *_abs functions give the
matrix products of absolute values the error bounds of tests/test_dense_grad_gpu.py are built on."""
import numpy as np


def _f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def masked_dy(dy, y_relu=None):
    dy = _f64(dy)
    return dy if y_relu is None else np.where(_f64(y_relu) > 0, dy, 0.0)


def dgrad(dy, w, y_relu=None, x_relu=None):
    dx = masked_dy(dy, y_relu) @ _f64(w)
    return dx if x_relu is None else np.where(_f64(x_relu) > 0, dx, 0.0)


def wgrad(dy, x, y_relu=None):
    dz = masked_dy(dy, y_relu)
    return dz.T @ _f64(x), dz.sum(axis=0)


def dgrad_abs(dy, w, y_relu=None):
    """|dz| . |w| [rows, cin]"""
    return np.abs(masked_dy(dy, y_relu)) @ np.abs(_f64(w))


def wgrad_abs(dy, x, y_relu=None):
    """(|dz|^T . |x| [cout, cin], column sums of |dz| [cout])"""
    dz = np.abs(masked_dy(dy, y_relu))
    return dz.T @ np.abs(_f64(x)), dz.sum(axis=0)
