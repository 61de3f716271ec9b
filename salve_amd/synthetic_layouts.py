"""Seeded synthetic room layouts for tests and measurements of the layout modality (beside salve_amd/synthetic.py, whose panoramas
and hypothesis tables they go with): rectangular and L-shaped rooms of 4 to 12 vertices with 0 to 6 windows, doors and openings on
their walls, a few panoramas without any, and one panorama whose room is empty."""

from __future__ import annotations

from typing import List

import numpy as np

from salve_amd.layout import WDO_TYPES, LayoutSpec, PanoLayouts

DRAW_ORDER = ("doors", "windows", "openings")   # layout_pair_specs' order


def make_layout_specs(n_panos: int, seed: int = 0) -> List[LayoutSpec]:
    """One closed-room LayoutSpec per panorama, metres in the panorama's own frame (the camera inside the room, near the origin).
    Panorama 1 (if there is one) has an EMPTY room; panoramas 2, 5, 8, ... have a room without W/D/Os."""
    rng = np.random.default_rng(seed)
    specs: List[LayoutSpec] = []
    for p in range(n_panos):
        if p == 1:
            specs.append((np.zeros((0, 2)), []))
            continue
        w, h = rng.uniform(1.0, 3.0, size=2)   # half extents; x 1.5 (HoHoNet -> ZInD) they reach 4.5 m of the window's 5
        c = rng.uniform(-0.4, 0.4, size=2)
        if p % 2 == 0:   # rectangle, counter-clockwise
            ring = np.array([[-w, -h], [w, -h], [w, h], [-w, h]])
        else:            # L shape: the rectangle with its top-right corner cut out
            a, b = rng.uniform(0.2, 0.8, size=2)
            ring = np.array([[-w, -h], [w, -h], [w, -h + 2 * h * b], [-w + 2 * w * a, -h + 2 * h * b], [-w + 2 * w * a, h], [-w, h]])
        # extra vertices on the walls (layout estimates carry them): up to 12 vertices in all
        for _ in range(int(rng.integers(0, 12 - len(ring) + 1))):
            k = int(rng.integers(0, len(ring)))
            u = rng.uniform(0.2, 0.8)
            ring = np.insert(ring, k + 1, ring[k] + u * (ring[(k + 1) % len(ring)] - ring[k]), axis=0)
        ring = ring + c
        wdos = []
        n_wdo = 0 if p % 3 == 2 else int(rng.integers(0, 7))
        kinds = sorted((DRAW_ORDER[int(k)] for k in rng.integers(0, 3, size=n_wdo)), key=DRAW_ORDER.index)
        for kind in kinds:
            k = int(rng.integers(0, len(ring)))
            a0, a1 = ring[k], ring[(k + 1) % len(ring)]
            u0 = rng.uniform(0.05, 0.6)
            u1 = u0 + rng.uniform(0.1, 0.35)
            wdos.append((kind, np.stack([a0 + u0 * (a1 - a0), a0 + u1 * (a1 - a0)])))
        specs.append((np.vstack([ring, ring[:1]]), wdos))
    assert all(t in WDO_TYPES for _, ws in specs for t, _ in ws)
    return specs


def make_layouts(n_panos: int, seed: int = 0) -> PanoLayouts:
    return PanoLayouts.from_specs(make_layout_specs(n_panos, seed))
