"""salve_amd.jpeg.HeaderCache without a GPU: `parse` is `parse_file` under the cache's options for every input -- files whose header
the cache has met (the marker walk skipped), headers it has not met, files damaged behind a known header -- and the refusals of the
`read_ahead` switch in the library and on the command line.

| what                                   | files                                                                                         |
|----------------------------------------|-----------------------------------------------------------------------------------------------|
| known header == cold parse_file        | the four fixture tiles; jpeg_cases' table through jpeg_decode_cases.pillow_file; every file of |
|                                        | jpeg_lanes_cases (restart=True) and of jpeg_sampling_cases (restart=True, every sampling)     |
| unknown header -> the full walk        | another quality, another size, a DRI segment, progressive, greyscale                          |
| damage behind a known header           | no EOI, a marker in the scan, cut behind the header, RSTn out of order, one interval too few  |
| options belong to the cache            | restart, samplings; a bad `samplings` is refused when the cache is made                       |
| the walk runs once per header          | 50 files of one header, `_walk_header` counted; 8 threads on one cache                        |
"""

import concurrent.futures
from pathlib import Path

import numpy as np
import pytest

import jpeg_cases as jc
import jpeg_decode_cases as dc
import jpeg_lanes_cases as lc
import jpeg_sampling_cases as sc
from salve_amd import jpeg

RENDERINGS = Path(__file__).resolve().parent / "golden" / "renderings"


def _outcome(fn, data):
    """("ok", ParsedFile) or ("unsupported", message)."""
    try:
        return "ok", fn(data)
    except jpeg.Unsupported as e:
        return "unsupported", str(e)


def _assert_same(got, want, what=""):
    assert got[0] == want[0], (what, got, want)
    if want[0] == "unsupported":
        assert got[1] == want[1], what
        return
    a, b = got[1], want[1]
    assert type(a) is type(b) is jpeg.ParsedFile
    for name in jpeg.ParsedFile._fields:
        x, y = getattr(a, name), getattr(b, name)
        if isinstance(y, np.ndarray):
            assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y), (what, name)
        else:
            assert type(x) is type(y) and x == y, (what, name)


def _check_group(files, **options):
    """One cache over the files twice: the first pass meets the headers, the second knows them all; both equal a cold parse_file."""
    cache = jpeg.HeaderCache(**options)
    cold = [_outcome(lambda d: jpeg.parse_file(d, **options), f) for f in files]
    for which in ("first pass", "second pass"):
        for i, f in enumerate(files):
            _assert_same(_outcome(cache.parse, f), cold[i], f"{which}, file {i}")
    return cache, cold


def _fixtures():
    return [p.read_bytes() for p in sorted(RENDERINGS.rglob("*.jpg"))]


def test_fixture_tiles_and_the_decode_table_equal_a_cold_parse():
    fixtures = _fixtures()
    assert len(fixtures) == 4
    cache, cold = _check_group(fixtures)
    assert all(c[0] == "ok" for c in cold) and len(cache) == 1          # one program wrote them: one header
    files = [dc.pillow_file(jc.make_image(c, h, w), quality=q) for c, h, w, q in jc.cases()]
    cache, cold = _check_group(files)
    assert all(c[0] == "ok" for c in cold)
    assert len(cache) == len({(h, w, q) for _, h, w, q in jc.cases()})   # a header per size and quality, shared by the contents


@pytest.mark.parametrize("restart", [True, False])
def test_the_lanes_table_equals_a_cold_parse(restart):
    files = [lc.file_of(name) for name in lc.cases()]
    _, cold = _check_group(files, restart=restart)
    refused = [name for name, c in zip(lc.cases(), cold) if c[0] == "unsupported"]
    assert refused == ([] if restart else [n for n in lc.cases() if n.startswith("restart_")])


def test_the_sampling_table_equals_a_cold_parse():
    files = [sc.file_of(s, name) for s, name in sc.cases()]
    _, cold = _check_group(files, restart=True, samplings=jpeg.SAMPLINGS)
    assert all(c[0] == "ok" for c in cold)
    assert {c[1].sampling for c in cold} == set(jpeg.SAMPLINGS)
    _check_group(files, restart=True, samplings=("4:2:2", "grey"))       # most are refused: the same messages
    _check_group(files)


def test_unknown_headers_fall_through_to_the_full_walk():
    rgb = jc.make_image("disc", 48, 64)
    known = dc.pillow_file(rgb, quality=75)
    others = {
        "another quality": dc.pillow_file(rgb, quality=60),
        "another size": dc.pillow_file(jc.make_image("disc", 48, 80), quality=75),
        "a DRI segment": dc.pillow_file(rgb, quality=75, restart_marker_blocks=2),
        "progressive": dc.pillow_file(rgb, quality=75, progressive=True),
        "greyscale": sc.pillow_file(rgb, "grey", quality=75),
    }
    for options in (dict(), dict(restart=True), dict(restart=True, samplings=jpeg.SAMPLINGS)):
        cache = jpeg.HeaderCache(**options)
        cache.parse(known)
        for what, data in others.items():
            want = _outcome(lambda d: jpeg.parse_file(d, **options), data)
            _assert_same(_outcome(cache.parse, data), want, what)
            _assert_same(_outcome(cache.parse, data), want, what + ", again")
    cache = jpeg.HeaderCache()
    for what in ("a DRI segment", "progressive", "greyscale"):
        assert _outcome(cache.parse, others[what])[0] == "unsupported", what
    assert len(cache) == 0                                               # a refused header leaves no entry


def test_damage_behind_a_known_header_gives_parse_files_message():
    good = _fixtures()[0]
    p = jpeg.parse_file(good)
    middle = p.scan_offset + p.scan_bytes // 2
    damaged = {
        "no EOI": good[:-2],
        "a marker inside the scan": good[:middle] + b"\xff\xd0" + good[middle:],
        "cut right behind the header": good[:p.scan_offset],
    }
    cache = jpeg.HeaderCache()
    cache.parse(good)
    for what, data in damaged.items():
        want = _outcome(jpeg.parse_file, data)
        assert want[0] == "unsupported", what
        _assert_same(_outcome(cache.parse, data), want, what)
    assert len(cache) == 1

    rst = lc.file_of("restart_blocks1")
    q = jpeg.parse_file(rst, restart=True)
    assert len(q.segments) == 12
    first_marker = q.segments[1][0] - 2
    last_marker = q.segments[-1][0] - 2
    assert rst[first_marker:first_marker + 2] == b"\xff\xd0"
    damaged = {
        "a wrong RSTn order": rst[:first_marker] + b"\xff\xd3" + rst[first_marker + 2:],
        "a wrong interval count": rst[:last_marker] + rst[last_marker + 2:],
        "no EOI": rst[:-2],
    }
    cache = jpeg.HeaderCache(restart=True)
    cache.parse(rst)
    messages = set()
    for what, data in damaged.items():
        want = _outcome(lambda d: jpeg.parse_file(d, restart=True), data)
        assert want[0] == "unsupported", what
        messages.add(want[1])
        _assert_same(_outcome(cache.parse, data), want, what)
    assert len(messages) == 3 and len(cache) == 1


def test_a_caches_options_cannot_be_bypassed():
    rst = lc.file_of("restart_blocks7")
    taking = jpeg.HeaderCache(restart=True)
    assert taking.parse(rst).segments == jpeg.parse_file(rst, restart=True).segments
    refusing = jpeg.HeaderCache(restart=False)
    for _ in range(2):
        with pytest.raises(jpeg.Unsupported, match="a restart interval"):
            refusing.parse(rst)
    full = sc.file_of("4:4:4", "24x40_disc")
    assert jpeg.HeaderCache(samplings=jpeg.SAMPLINGS).parse(full).sampling == "4:4:4"
    with pytest.raises(jpeg.Unsupported) as cold:
        jpeg.parse_file(full)
    narrow = jpeg.HeaderCache()
    for _ in range(2):
        with pytest.raises(jpeg.Unsupported) as cached:
            narrow.parse(full)
        assert str(cached.value) == str(cold.value)
    assert (refusing.restart, refusing.samplings) == (False, ("4:2:0",))
    for bad in ((), ("4:1:1",), ("4:2:0", "colour")):
        with pytest.raises(ValueError, match="samplings"):
            jpeg.HeaderCache(samplings=bad)


def test_the_marker_walk_runs_once_per_header(monkeypatch):
    files = [dc.pillow_file(jc.make_image("noise", 16, 16, seed), quality=75) for seed in range(50)]
    assert len(set(files)) == 50
    calls = []
    walk = jpeg._walk_header

    def counted(*a):
        calls.append(1)
        return walk(*a)

    monkeypatch.setattr(jpeg, "_walk_header", counted)
    cache = jpeg.HeaderCache()
    parsed = [cache.parse(f) for f in files]
    assert len(calls) == 1 and len(cache) == 1
    for f in files:
        jpeg.parse_file(f)
    assert len(calls) == 51                                              # (parse_file takes the same walk: the count sees it)
    monkeypatch.undo()
    for f, got in zip(files, parsed):
        _assert_same(("ok", got), ("ok", jpeg.parse_file(f)))


def test_one_cache_serves_several_threads():
    files = [dc.pillow_file(jc.make_image("noise", h, 16, seed), quality=75) for seed in range(40) for h in (16, 24, 32)]
    cold = [("ok", jpeg.parse_file(f)) for f in files]
    cache = jpeg.HeaderCache()
    with concurrent.futures.ThreadPoolExecutor(max_workers=8) as pool:
        got = list(pool.map(cache.parse, files * 3))
    assert len(cache) == 3
    for i, g in enumerate(got):
        _assert_same(("ok", g), cold[i % len(files)], f"file {i}")


def test_read_ahead_is_refused_without_the_device_decoder(capsys):
    from salve_amd import evaluate, train as train_cli, train_utils, training

    with pytest.raises(ValueError, match="read_ahead"):
        training.train(None, "unused", decode="host", read_ahead=True)
    with pytest.raises(ValueError, match="read_ahead"):
        train_utils.get_dataloader(None, "val", decode="host", read_ahead=True)
    with pytest.raises(ValueError, match="read_ahead"):
        evaluate.evaluate_model("unused", "unused.pth", None, "val", read_ahead=True)
    with pytest.raises(SystemExit, match="--decode-read-ahead"):
        train_cli.main(["--config", "unused.yaml", "--decode-read-ahead"])
    with pytest.raises(SystemExit, match="--decode-read-ahead"):
        train_cli.main(["--config", "unused.yaml", "--decode", "host", "--decode-read-ahead"])
    with pytest.raises(SystemExit, match="--prefetch"):                  # --prefetch keeps its own refusal beside the new flag
        train_cli.main(["--config", "unused.yaml", "--decode", "device", "--decode-read-ahead", "--prefetch"])
    with pytest.raises(SystemExit) as done:
        train_cli.main(["--help"])
    assert done.value.code == 0 and "--decode-read-ahead" in capsys.readouterr().out
