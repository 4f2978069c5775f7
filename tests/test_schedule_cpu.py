"""Host side of the hyper-parameter schedules (no GPU): the two device-hyper entry points are declared, exported and in
the ctypes table, reject a NULL hyper pointer, and the values staged for them are validated on the host."""
import ctypes
import math

import pytest
import torch


@pytest.fixture(scope="module")
def built():
    from hashmodnffbanks_idr_amd import build
    return build.build(verbose=False)


NEW = ("hm_adam_step_dev", "hm_idr_loss_dev")


def test_device_hyper_entry_points_are_declared_exported_and_bound(built):
    import os
    import re
    from hashmodnffbanks_idr_amd._lib import SIGNATURES
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "hashmod.h")).read()
    L = ctypes.CDLL(built)
    for name in NEW:
        assert re.search(r"HM_API int " + name + r"\(", header), name
        assert hasattr(L, name), name
        assert name in SIGNATURES, name


def test_null_hyper_pointer_is_invalid(built):
    from hashmodnffbanks_idr_amd import _lib
    L = _lib.lib()
    fake = ctypes.c_void_p(4096)      # never dereferenced: the argument checks return first
    rc = L.hm_adam_step_dev(None, 0, None, 1, fake, None)
    assert rc == -1 and b"hyper" in L.hm_last_error()
    with pytest.raises(ValueError):
        _lib.check(rc)
    rc = L.hm_idr_loss_dev(fake, fake, fake, fake, fake, 1, None, 0, None, fake, fake, fake, None, None)
    assert rc == -1 and b"hyper" in L.hm_last_error()
    with pytest.raises(ValueError):
        _lib.check(rc)


def _opt(**kw):
    from hashmodnffbanks_idr_amd.training.optim import ClipAdam
    return ClipAdam([torch.nn.Parameter(torch.zeros(3))], **kw)


def test_clip_adam_hyper_values():
    opt = _opt(lr=2e-4, betas=(0.8, 0.99), eps=1e-7, max_norm=None)
    assert opt.hyper_values() == [2e-4, 0.8, 0.99, 1e-7, 0.0]
    opt.max_norm = 1.0
    opt.param_groups[0]["lr"] = torch.tensor(5e-5)      # a scheduler may leave a tensor
    assert opt.hyper_values() == [pytest.approx(5e-5), 0.8, 0.99, 1e-7, 1.0]


@pytest.mark.parametrize("key,value", [("lr", -1e-4), ("lr", math.nan), ("betas", (1.0, 0.999)),
                                       ("betas", (0.9, -0.1)), ("eps", -1e-8)])
def test_clip_adam_rejects_invalid_values(key, value):
    opt = _opt()
    opt.param_groups[0][key] = value
    with pytest.raises(ValueError):
        opt.hyper_values()


def test_clip_adam_rejects_what_it_does_not_implement():
    opt = _opt()
    opt.param_groups[0]["weight_decay"] = 1e-2
    with pytest.raises(NotImplementedError):
        opt.hyper_values()


def test_clip_adam_captured_without_clipping_cannot_turn_it_on():
    opt = _opt(max_norm=0.0)
    opt._captured_clip = False          # what step() records when it is captured with max_norm 0
    assert opt.hyper_values(captured=True)[4] == 0.0
    opt.max_norm = 1.0
    assert opt.hyper_values()[4] == 1.0                 # an eager step can clip
    with pytest.raises(RuntimeError, match="max_norm"):
        opt.hyper_values(captured=True)
    with pytest.raises(RuntimeError, match="load_state_dict"):
        opt.load_state_dict(opt.state_dict())


def test_loss_hyper_values():
    from hashmodnffbanks_idr_amd.model.loss import loss_hyper_values
    assert loss_hyper_values(0.1, 100, 50) == [0.1, 100.0, 50.0]
    for bad in ((0.1, 100.0, 0.0), (0.1, 100.0, -2.0), (0.1, 100.0, math.nan), (math.nan, 1.0, 1.0)):
        with pytest.raises(ValueError):
            loss_hyper_values(*bad)


def test_torch_adam_hyper_changes_are_caught_tensors_are_followed():
    from hashmodnffbanks_idr_amd.training.graph_step import _same_value
    lr = torch.tensor(1e-4)
    assert _same_value(lr, lr) and not _same_value(lr, torch.tensor(1e-4))
    assert _same_value((0.9, 0.999), (0.9, 0.999)) and not _same_value((0.9, 0.999), (0.8, 0.999))
    assert not _same_value(1e-4, 5e-5) and _same_value(None, None)
