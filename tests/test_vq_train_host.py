"""CPU checks of the training-mode VQ boundary: the EMA-update entry points are
exported and validate their arguments before any device work, the stage-1
trainer exists with the reference's constructor, and the quantizer module has
no torch EMA path left."""
import ctypes
import inspect

import pytest

N, D, S, K = 64, 64, 3, 256


class Stage(ctypes.Structure):  # sel_rvq_ema_stage (include/sel.h)
    _fields_ = [("embed", ctypes.c_void_p), ("cluster_size", ctypes.c_void_p), ("embed_avg", ctypes.c_void_p),
                ("update", ctypes.c_int32), ("reserved", ctypes.c_int32)]


@pytest.fixture(scope="module")
def lib():
    from sel import _lib
    return _lib.load()


def test_ema_symbols_exported(lib):
    from sel import _lib
    for name in ("sel_rvq_ema_workspace", "sel_rvq_ema_update"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert ctypes.sizeof(Stage) == 32


def _update(lib, n=N, d=D, s=S, k=K, ws_bytes=None, table=True):
    """Every device pointer is null, so no call here can reach the device even
    if a check were missing: the shape, the workspace and the table are checked
    before the pointers, and each refusal names what it refused."""
    tab = (Stage * 16)()
    need = lib.sel_rvq_ema_workspace(max(n, 1), min(d, 256), min(s, 16), k)
    return lib.sel_rvq_ema_update(None, n, d, None, s, k, None, None,
                                  ctypes.cast(tab, ctypes.c_void_p) if table else None, 0.8, 1e-5, None,
                                  need if ws_bytes is None else ws_bytes, None)


@pytest.mark.parametrize("case, kwargs, says", [
    ("N = 0", dict(n=0), "N=0"),
    ("D = 257", dict(d=257), "D=257"),
    ("S = 17", dict(s=17), "S=17"),
    ("short workspace", dict(ws_bytes=N * D * S * 4 - 1), "workspace"),
    ("null table", dict(table=False), "table"),
])
def test_ema_update_refuses_before_device_work(lib, case, kwargs, says):
    rc = _update(lib, **kwargs)
    assert rc < 0, case
    assert says in lib.sel_last_error().decode(), (case, lib.sel_last_error())


def test_ema_workspace_monotone_in_rows(lib):
    sizes = [lib.sel_rvq_ema_workspace(n, D, S, K) for n in (1, 2, 15, 16, 17, 150, 512, 5120, 1 << 20)]
    assert sizes == sorted(sizes) and sizes[0] > 0 and sizes[-1] > sizes[0]
    assert lib.sel_rvq_ema_workspace(5120, 64, 8, 1024) >= 5120 * 64 * 8 * 4   # the residuals, (S, N, D) fp32


def test_autoencoder_trainer_is_a_vqgan_trainer():
    from trainer.autoencoder import Trainer
    from trainer.trainerGAN import TrainerVQGAN
    assert issubclass(Trainer, TrainerVQGAN)
    sig = inspect.signature(Trainer.__init__)
    assert list(sig.parameters) == ["self", "steps", "epochs", "data_loader", "model", "criterion", "optimizer",
                                    "scheduler", "config", "device"]
    assert str(sig.parameters["device"].default) == "cpu"
    tr = Trainer(0, 0, {}, {}, {}, {}, {}, {})
    assert (tr.paradigm, tr.generator_start, tr.discriminator_start, tr.fix_encoder) == ("efficient", 0, 200000, False)
    tr = Trainer(0, 0, {}, {}, {}, {}, {}, {"paradigm": "x", "start_steps": {"generator": 3, "discriminator": 5}})
    assert (tr.paradigm, tr.generator_start, tr.discriminator_start) == ("x", 3, 5)


def test_vector_quantize_has_no_torch_ema_path():
    from layers import vq_module
    assert not hasattr(vq_module.VectorQuantize, "_ema")
    src = inspect.getsource(vq_module)
    for op in ("bincount", "index_add", "mse_loss"):
        assert op not in src, op
