"""Pixels of an equirectangular panorama -> metres on the floor plane: the reference's salve/utils/zind_pano_utils.py:35-200
(`convert_points_px_to_worldmetric` = zind_pixel_to_sphere, zind_sphere_to_cartesian, zind_room_cartesian_to_worldmetric) restated in plain
numpy, operation by operation.  Host only: MHNet's floor boundary and W/D/O columns become a panorama's layout with it
(salve_amd/dataset/mhnet_prediction.py)."""

from __future__ import annotations

import math

import numpy as np

EPS_RAD = 1e-10


def convert_points_px_to_worldmetric(points_px: np.ndarray, image_width: int, camera_height_m: float) -> np.ndarray:
    """points_px [N, 2] (x in [0, width), y >= 0) -> [N, 3] world-metric coordinates of the floor points seen there, z = the vertical axis.
    The reference's steps, in its order: x / (width - 1) and y / (height - 1) with height = width / 2 (:66, :85, :91); a y >= height is clipped
    to height - 1 (:76-79); theta in [-pi, pi], phi in [-pi / 2, pi / 2]; the unit ray (:148-152); z flipped, the ray scaled so that |y| is the
    camera height (:170-174); y and z swapped and x negated (:177-180)."""
    points_px = np.asarray(points_px)
    if points_px.ndim != 2 or points_px.shape[1] != 2:
        raise RuntimeError(f"Input shape should have been (N,2), but received {points_px.shape}")
    if len(points_px) == 0:
        raise ValueError("convert_points_px_to_worldmetric needs at least one point")
    width = image_width
    height = width / 2
    if not (width > 1 and height > 1):
        raise ValueError(f"image width {width} is too small")
    x_arr = points_px[:, 0]
    y_arr = points_px[:, 1]
    if not (np.all(np.greater_equal(x_arr, 0.0)) and np.all(np.less(x_arr, width)) and np.all(np.greater_equal(y_arr, 0.0))):
        raise ValueError(f"pixel coordinates outside the panorama: x must lie in [0, {width}) and y must not be negative")
    if not np.all(np.less(y_arr, height)):
        y_arr = np.clip(y_arr, a_min=0, a_max=height - 1)
    theta = x_arr / (width - 1)
    theta = theta * (2.0 * math.pi)
    theta = theta - math.pi
    phi = y_arr / (height - 1)
    phi = 1.0 - phi
    phi = phi * math.pi
    phi = phi - math.pi / 2.0
    if not np.all(np.greater_equal(phi, -math.pi / 2.0 - EPS_RAD)):
        phi = np.clip(phi, a_min=-np.pi / 2, a_max=np.pi / 2)
    rho = np.ones_like(theta)
    rho_cos_phi = rho * np.cos(phi)
    cart = np.column_stack((rho_cos_phi * np.sin(theta), rho * np.sin(phi), rho_cos_phi * np.cos(theta)))
    cart[:, 2] *= -1
    world = cart / cart[:, 1].reshape(-1, 1)
    world *= camera_height_m
    world = world[:, np.array([0, 2, 1])]
    world[:, 0] *= -1
    return world
