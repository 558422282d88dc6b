"""examples/BERT/bert_train.py sizes the position table for sequences beyond BERT-base's 512 positions."""
import importlib.util
import os
import sys

import pytest

HERE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "BERT")


@pytest.mark.parametrize("argv,want", [([], 512), (["--seq", "512"], 512), (["--seq", "1024"], 1024),
                                       (["--seq", "1024", "--max_position", "2048"], 2048),
                                       (["--tiny", "--seq", "1024"], 64)])
def test_max_position_follows_seq(argv, want, monkeypatch):
    monkeypatch.syspath_prepend(HERE)  # the script's ``import _path``
    spec = importlib.util.spec_from_file_location("bert_train_under_test", os.path.join(HERE, "bert_train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    sys.modules.pop("_path", None)
    assert mod.model_config(mod.parse_args(argv)).max_position == want
