"""The optimizer configuration of the fused device step for the kinds beyond SGD and Adam — AdamW, RMSprop, Adagrad, Adamax
(`native.make_opt_cfg`, `bsvi_opt_cfg` in include/bsvi.h): how torch's keyword arguments land in the words of the struct, torch's
defaults, the options and ranges that are refused, and that neither the struct's layout nor the ABI number moved.  No GPU."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

from brancher_amd import native, workloads as W
from brancher_amd.optimizers import ProbabilisticOptimizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORDS = [name for name, _ in native.OptCfg._fields_]


def words(cfg):
    return {name: getattr(cfg, name) for name in WORDS}


def f32(v):
    return C.c_float(v).value


def test_adamw_maps_as_adam_with_its_own_kind():
    cfg = native.make_opt_cfg("AdamW", lr=3e-3, betas=(0.8, 0.95), eps=1e-6, weight_decay=0.1, amsgrad=True, maximize=True)
    assert words(cfg) == dict(kind=2, lr=f32(3e-3), momentum=0.0, dampening=0.0, weight_decay=f32(0.1), nesterov=0, beta1=f32(0.8),
                              beta2=f32(0.95), eps=f32(1e-6), amsgrad=1, maximize=1)


def test_rmsprop_mapping():
    cfg = native.make_opt_cfg("RMSprop", lr=3e-3, alpha=0.9, eps=1e-6, weight_decay=0.1, momentum=0.7, centered=True, maximize=True)
    assert words(cfg) == dict(kind=3, lr=f32(3e-3), momentum=f32(0.7), dampening=0.0, weight_decay=f32(0.1), nesterov=0, beta1=0.0,
                              beta2=f32(0.9), eps=f32(1e-6), amsgrad=1, maximize=1)


def test_adagrad_mapping():
    cfg = native.make_opt_cfg("Adagrad", lr=3e-3, lr_decay=0.05, weight_decay=0.1, initial_accumulator_value=0.3, eps=1e-6, maximize=True)
    assert words(cfg) == dict(kind=4, lr=f32(3e-3), momentum=0.0, dampening=f32(0.05), weight_decay=f32(0.1), nesterov=0,
                              beta1=f32(0.3), beta2=0.0, eps=f32(1e-6), amsgrad=0, maximize=1)


def test_adamax_mapping():
    cfg = native.make_opt_cfg("Adamax", lr=3e-3, betas=[0.8, 0.95], eps=1e-6, weight_decay=0.1, maximize=True)
    assert words(cfg) == dict(kind=5, lr=f32(3e-3), momentum=0.0, dampening=0.0, weight_decay=f32(0.1), nesterov=0, beta1=f32(0.8),
                              beta2=f32(0.95), eps=f32(1e-6), amsgrad=0, maximize=1)


# torch keyword -> the word of bsvi_opt_cfg that carries it (the table at bsvi_opt_cfg, include/bsvi.h)
FIELD_OF = {
    "AdamW": dict(lr="lr", betas=("beta1", "beta2"), eps="eps", weight_decay="weight_decay", amsgrad="amsgrad", maximize="maximize"),
    "RMSprop": dict(lr="lr", alpha="beta2", eps="eps", weight_decay="weight_decay", momentum="momentum", centered="amsgrad",
                    maximize="maximize"),
    "Adagrad": dict(lr="lr", lr_decay="dampening", weight_decay="weight_decay", initial_accumulator_value="beta1", eps="eps",
                    maximize="maximize"),
    "Adamax": dict(lr="lr", betas=("beta1", "beta2"), eps="eps", weight_decay="weight_decay", maximize="maximize"),
}
NOT_IMPLEMENTED = ("foreach", "fused", "capturable", "differentiable")


@pytest.mark.parametrize("name", sorted(FIELD_OF))
def test_defaults_are_torchs(name):
    cfg = native.make_opt_cfg(name)
    signature = inspect.signature(getattr(torch.optim, name).__init__).parameters
    seen = set()
    for option, field in FIELD_OF[name].items():
        default = signature[option].default
        if isinstance(field, tuple):
            for f, d in zip(field, default):
                assert getattr(cfg, f) == f32(d), (name, option)
        else:
            assert getattr(cfg, field) == (f32(default) if isinstance(default, float) else int(default)), (name, option)
        seen.add(option)
    # every option of torch's constructor is either mapped or one of those the step does not implement
    assert set(signature) - {"self", "params"} - seen <= set(NOT_IMPLEMENTED), name
    assert native.make_opt_cfg("AdamW").weight_decay == f32(1e-2)
    assert native.make_opt_cfg("Adagrad").eps == f32(1e-10) and native.make_opt_cfg("Adagrad").lr == f32(1e-2)
    assert native.make_opt_cfg("RMSprop").beta2 == f32(0.99) and native.make_opt_cfg("RMSprop").lr == f32(1e-2)
    assert native.make_opt_cfg("Adamax").lr == f32(2e-3)


@pytest.mark.parametrize("name", sorted(FIELD_OF))
@pytest.mark.parametrize("option", NOT_IMPLEMENTED + ("no_such_option",))
def test_unsupported_and_unknown_options_are_named(name, option):
    with pytest.raises(NotImplementedError, match=option):
        native.make_opt_cfg(name, lr=1e-3, **{option: True})


def test_options_of_another_kind_are_refused():
    for name, kw in (("AdamW", dict(alpha=0.9)), ("RMSprop", dict(betas=(0.9, 0.99))), ("RMSprop", dict(amsgrad=True)),
                     ("Adagrad", dict(momentum=0.5)), ("Adamax", dict(amsgrad=True)), ("Adamax", dict(centered=True))):
        with pytest.raises(NotImplementedError, match=list(kw)[0]):
            native.make_opt_cfg(name, **kw)


@pytest.mark.parametrize("name,kw", [
    ("AdamW", dict(lr=-1e-3)), ("AdamW", dict(eps=-1e-8)), ("AdamW", dict(weight_decay=-0.1)),
    ("AdamW", dict(betas=(1.0, 0.999))), ("AdamW", dict(betas=(0.9, -0.1))),
    ("RMSprop", dict(lr=-1e-3)), ("RMSprop", dict(eps=-1e-8)), ("RMSprop", dict(weight_decay=-0.1)), ("RMSprop", dict(alpha=-0.5)),
    ("RMSprop", dict(momentum=-0.5)),
    ("Adagrad", dict(lr=-1e-3)), ("Adagrad", dict(eps=-1e-8)), ("Adagrad", dict(weight_decay=-0.1)), ("Adagrad", dict(lr_decay=-0.1)),
    ("Adagrad", dict(initial_accumulator_value=-0.1)),
    ("Adamax", dict(lr=-1e-3)), ("Adamax", dict(eps=-1e-8)), ("Adamax", dict(weight_decay=-0.1)), ("Adamax", dict(betas=(0.9, 1.0))),
    ("Adamax", dict(betas=(-0.1, 0.9))),
])
def test_out_of_range_values_raise_as_in_torch(name, kw):
    with pytest.raises(ValueError):
        getattr(torch.optim, name)([torch.zeros(1, requires_grad=True)], **kw)
    with pytest.raises(ValueError):
        native.make_opt_cfg(name, **kw)


@pytest.mark.parametrize("name", ["NAdam", "LBFGS", "RAdam", "Adadelta"])
def test_other_optimizers_stay_refused_and_the_message_lists_the_six(name):
    with pytest.raises(NotImplementedError) as err:
        native.make_opt_cfg(name, lr=1e-3)
    for served in ("SGD", "Adam", "AdamW", "RMSprop", "Adagrad", "Adamax"):
        assert served in str(err.value)


def test_sgd_and_adam_configurations_are_as_they_were():
    assert words(native.make_opt_cfg("SGD", lr=0.1, momentum=0.9, nesterov=True)) == dict(
        kind=0, lr=f32(0.1), momentum=f32(0.9), dampening=0.0, weight_decay=0.0, nesterov=1, beta1=0.0, beta2=0.0, eps=0.0, amsgrad=0,
        maximize=0)
    assert words(native.make_opt_cfg("Adam", lr=0.1, betas=(0.8, 0.9), amsgrad=True)) == dict(
        kind=1, lr=f32(0.1), momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=0, beta1=f32(0.8), beta2=f32(0.9), eps=f32(1e-8),
        amsgrad=1, maximize=0)


def test_header_enum_equals_the_python_constants():
    text = open(os.path.join(ROOT, "include", "bsvi.h")).read()
    body = re.search(r"typedef enum bsvi_optimizer_kind \{(.*?)\}", text, re.S).group(1)
    enum = {k: int(v) for k, v in re.findall(r"(BSVI_OPT_\w+)\s*=\s*(\d+)", body)}
    assert enum == dict(BSVI_OPT_SGD=native.OPT_SGD, BSVI_OPT_ADAM=native.OPT_ADAM, BSVI_OPT_ADAMW=native.OPT_ADAMW,
                        BSVI_OPT_RMSPROP=native.OPT_RMSPROP, BSVI_OPT_ADAGRAD=native.OPT_ADAGRAD, BSVI_OPT_ADAMAX=native.OPT_ADAMAX)
    assert enum == {"BSVI_OPT_" + name.upper(): i for i, name in enumerate(native.OPTIMIZER_NAMES)}
    for i, name in enumerate(native.OPTIMIZER_NAMES):
        assert native.make_opt_cfg(name).kind == i


def test_layout_and_abi_are_unchanged():
    assert native.ABI_VERSION == 11
    assert C.sizeof(native.OptCfg) == 44 and len(WORDS) == 11
    assert WORDS == ["kind", "lr", "momentum", "dampening", "weight_decay", "nesterov", "beta1", "beta2", "eps", "amsgrad", "maximize"]
    assert [getattr(native.OptCfg, w).offset for w in WORDS] == [4 * i for i in range(11)]
    text = open(os.path.join(ROOT, "include", "bsvi.h")).read()
    assert re.search(r"#define\s+BSVI_ABI_VERSION\s+11\b", text)


def test_probabilistic_optimizer_records_a_configuration():
    model = W.build_beta_binomial(W.native_api(), n_obs=30)
    opt = ProbabilisticOptimizer(model.posterior_model, "RMSprop", lr=0.02, momentum=0.5)
    assert isinstance(opt.optimizer, native.OptCfg)
    assert opt.optimizer.kind == native.OPT_RMSPROP and opt.optimizer.lr == f32(0.02) and opt.optimizer.momentum == f32(0.5)
    assert isinstance(ProbabilisticOptimizer(model.posterior_model, "Adagrad", lr=0.05).optimizer, native.OptCfg)
