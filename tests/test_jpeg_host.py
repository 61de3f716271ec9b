"""The JPEG round trip on the host: the integer emulator of tests/jpeg_cases.py against Pillow, pixel for pixel on every case, the
quality tables against the ones Pillow's files carry, and four plausible wrong variants of the chain that the case table must tell
from the real one.  No device.

Sizes (h x w) and why: 1 x 1 the smallest image; 8 x 8 one DCT block (and an even height that is no multiple of 16: the downsampled
rows are replicated, not the full-resolution ones); 16 x 16 one MCU; 15 x 17 and 17 x 9 both edges partial; 33 x 47 interior MCU
borders in both directions and an odd chroma size; 501 x 501 the product's BEV size."""

import io

import numpy as np
import pytest

import jpeg_cases as jc
from salve_amd.jpeg import quality_tables

PIL_Image = pytest.importorskip("PIL.Image")

CASES = jc.cases()


def _id(case):
    return f"{case[0]}-{case[1]}x{case[2]}-q{case[3]}"


def test_the_case_table_is_the_one_the_tests_document():
    assert jc.SMALL_SIZES == ((1, 1), (8, 8), (16, 16), (15, 17), (17, 9), (33, 47)) and jc.PRODUCT_SIZE == (501, 501)
    assert jc.SMALL_QUALITIES == (75, 30, 95) and len(jc.CONTENTS) == 7
    assert len(CASES) == len(set(CASES)) == 6 * 3 * 7 + 7
    # the noise content saturates both range limits somewhere after the round trip
    out = jc.pillow_reference(("noise", 33, 47, 30))
    assert out.min() == 0 and out.max() == 255


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_emulator_equals_pillow(case):
    content, h, w, q = case
    got = jc.roundtrip(jc.make_image(content, h, w), quality_tables(q))
    want = jc.pillow_reference(case)
    assert got.shape == want.shape == (h, w, 3)
    assert int((got != want).any(-1).sum()) == 0


def _natural(table):
    """A quantisation table as Pillow reports it, in natural (row-major) order whichever order this Pillow reports."""
    t = np.asarray(table, dtype=np.int64)
    zigzag = np.array(sorted(range(64), key=lambda i: (i // 8 + i % 8, (i // 8) if (i // 8 + i % 8) % 2 else (i % 8))))   # natural index of zigzag k
    alt = np.empty(64, dtype=np.int64)
    alt[zigzag] = t
    return t, alt


@pytest.mark.parametrize("q", [1, 10, 30, 50, 75, 95, 100])
def test_quality_tables_equal_the_tables_in_pillows_files(q):
    buf = io.BytesIO()
    PIL_Image.fromarray(jc.make_image("noise", 16, 16)).save(buf, format="JPEG", quality=q)
    buf.seek(0)
    with PIL_Image.open(buf) as im:
        tables = im.quantization
    ours = quality_tables(q)
    assert ours.shape == (2, 64) and ours.dtype == np.uint16 and ours.min() >= 1 and ours.max() <= 255
    for k in range(2):
        as_reported, dezigzagged = _natural(tables[k])
        # a symmetric table reads the same both ways; the luma table is not symmetric and decides the order for both
        assert np.array_equal(ours[k], as_reported) or np.array_equal(ours[k], dezigzagged), (q, k)
    lum_reported, lum_dezigzagged = _natural(tables[0])
    natural = np.array_equal(ours[0], lum_reported)
    assert np.array_equal(ours[1], _natural(tables[1])[0 if natural else 1])


def test_quality_is_clamped_as_libjpeg_clamps_it():
    assert np.array_equal(quality_tables(0), quality_tables(1)) and np.array_equal(quality_tables(-5), quality_tables(1))
    assert np.array_equal(quality_tables(101), quality_tables(100)) and int(quality_tables(100).max()) == 1
    assert int(quality_tables(1).max()) == 255   # forced baseline
    assert quality_tables(75)[0, :8].tolist() == [8, 6, 5, 8, 12, 20, 26, 31] and quality_tables(75)[1, :8].tolist() == [9, 9, 12, 24, 50, 50, 50, 50]


@pytest.mark.parametrize("mutant", jc.MUTANTS)
def test_a_wrong_variant_changes_at_least_one_case(mutant):
    small = [c for c in CASES if c[1] <= 47]
    changed = [c for c in small if not np.array_equal(jc.roundtrip(jc.make_image(*c[:3]), quality_tables(c[3]), mutant=mutant), jc.pillow_reference(c))]
    assert changed, f"no case tells the '{mutant}' variant from libjpeg's chain"
