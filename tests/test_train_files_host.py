"""decode="device" without a GPU: the switch's refusals on the command line and in the library."""

import pytest

from salve_amd import train as train_cli
from salve_amd import training


def test_decode_device_is_refused_together_with_render_from():
    with pytest.raises(SystemExit, match="--render-from"):
        train_cli.main(["--config", "unused.yaml", "--decode", "device", "--render-from", "/nonexistent"])
    with pytest.raises(SystemExit):   # argparse: not one of the choices
        train_cli.main(["--config", "unused.yaml", "--decode", "gpu"])


def test_unknown_decode_values_are_refused():
    with pytest.raises(ValueError, match="decode"):
        training._check_decode("gpu")
    for ok in training.DECODES:
        training._check_decode(ok)
    assert training.DECODES == ("host", "device")
