"""The training step of the grasp-quality network without a GPU: tests/grasp_train_host.py -- the float32
restatement of csrc/rv_dev_grasp_train.h -- against an independent float64 backward pass with a derived bound (its
docstring), that float64 pass against torch's double autograd, two planted errors the bound must reject, Adam against
float64 and torch.optim.Adam, the blob round trip and the C layout."""
import ctypes as C
import os

import numpy as np
import pytest

import grasp_quality_host as gqh
import grasp_train_host as gth
from robovat_amd import abi, lib
from robovat_amd.perception import grasp_quality as gq
from robovat_amd.perception.grasp_quality import GraspQualityModel

HERE = os.path.dirname(os.path.abspath(__file__))
F = np.float32
NORM = dict(im_mean=0.45, im_inv_std=3.7, z_mean=0.55, z_inv_std=19.0)
MODELS = {
    'tiny': dict(gq.TINY_SIZES),
    '8x12': dict(height=8, width=12, c1=4, c2=8, f1=8, f2=4, p=4),
    'default': dict(gq.DEFAULT_SIZES),
}
COUNT = {'tiny': 16, '8x12': 16, 'default': 3}
SEEDS = (1, 2, 3)


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _model(name, seed=1):
    return GraspQualityModel.random_init(seed, norm=NORM, **MODELS[name])


def _case(name, seed):
    m = _model(name, seed)
    x, z = gqh.sample_inputs(seed, COUNT[name], m.sizes['height'], m.sizes['width'])
    g = np.random.RandomState(100 + seed).standard_normal(COUNT[name]).astype(F)
    return m, x, z, g


@pytest.fixture(scope='module')
def checked():
    """(name, seed) -> everything the gradient tests need, computed once: the samples whose masks agree, the restatement's
    gradients on them, the float64 gradients and bounds"""
    out = {}
    for name in MODELS:
        for seed in SEEDS:
            m, x, z, g = _case(name, seed)
            y32, a32 = gth.forward_train(m.params, m.norm, x, z)
            y64, B, a64 = gth.forward64_train(m.params, m.norm, x, z)
            keep = gth.masks_agree(a32, a64)
            a32k, a64k, gk = gth.take(a32, keep), gth.take(a64, keep), g[keep]
            grads = gth.backward(m.params, a32k, gk)
            G, Bd = gth.backward64(m.params, a64k, gk)
            out[name, seed] = dict(model=m, x=x, z=z, g=g, y32=y32, keep=keep, a32=a32k, a64=a64k, gk=gk, grads=grads, G=G, B=Bd)
    return out


def _worst(grads, G, B):
    """the largest |restatement - float64| / bound over every entry (0 / 0 counts as 0)"""
    worst = 0.0
    for k in gq.PARAM_NAMES:
        d = np.abs(grads[k].astype(np.float64) - G[k])
        assert d.shape == B[k].shape
        r = np.where(d > 0, d / np.where(B[k] > 0, B[k], 1e-300), 0.0)
        worst = max(worst, float(r.max()))
    return worst


@pytest.mark.parametrize('name', sorted(MODELS))
def test_forward_logits_are_the_forward_restatement_bit_for_bit(checked, name):
    for seed in SEEDS:
        c = checked[name, seed]
        m = c['model']
        assert np.array_equal(_bits(c['y32']), _bits(gqh.forward(m.params, m.norm, c['x'], c['z'])))
    # the chosen positions: a window with two equal positive maxima takes the first, an all-zero window takes 0
    r = np.zeros((1, 1, 4, 4), F)
    r[0, 0, 0, 1] = r[0, 0, 1, 0] = F(2.0)
    r[0, 0, 2, 3] = F(1.0); r[0, 0, 3, 3] = F(1.0)
    mx, s = gth.pool2_idx(r)
    assert mx.tolist() == [[[[2.0, 0.0], [0.0, 1.0]]]] and s.tolist() == [[[[1, 0], [0, 1]]]]


@pytest.mark.parametrize('name', sorted(MODELS))
def test_every_gradient_is_within_the_derived_bound_of_float64(checked, name):
    worst = 0.0
    for seed in SEEDS:
        c = checked[name, seed]
        left_out = int((~c['keep']).sum())
        assert 8 * left_out <= len(c['keep']), 'seed %d: %d of %d samples have other masks in float64' % (seed, left_out, len(c['keep']))
        for k in gq.PARAM_NAMES:
            assert c['grads'][k].dtype == F and c['grads'][k].shape == c['model'].params[k].shape
            assert np.abs(c['G'][k]).max() > 0, k
        w = _worst(c['grads'], c['G'], c['B'])
        print('%s seed %d: %d of %d samples left out, largest |restatement - float64| / bound = %.3e'
              % (name, seed, left_out, len(c['keep']), w))
        worst = max(worst, w)
    print('%s: largest ratio over the seeds %.3e' % (name, worst))
    assert worst <= 1.0


@pytest.mark.parametrize('name', sorted(MODELS))
def test_the_bound_rejects_two_planted_errors(checked, name):
    c = checked[name, 1]
    m = c['model']
    # conv2's weight gradient with ky and kx swapped
    bad = dict(c['grads'])
    bad['conv2.weight'] = np.ascontiguousarray(c['grads']['conv2.weight'].transpose(0, 1, 3, 2))
    assert _worst(bad, c['G'], c['B']) > 1.0
    # every pool gradient routed to v00 instead of the chosen position
    bad = gth.backward(m.params, c['a32'], c['gk'], route_v00=True)
    assert _worst(bad, c['G'], c['B']) > 1.0


@pytest.mark.parametrize('name', sorted(MODELS))
def test_float64_backward_agrees_with_torch_double_autograd(checked, name):
    import torch
    c = checked[name, 2]
    m = c['model']
    keep = c['keep']
    net = m.torch_module().double()
    x = torch.from_numpy(c['x'][keep].astype(np.float64))
    z = torch.from_numpy(c['z'][keep].astype(np.float64))
    logits = net(x, z)
    logits.backward(torch.from_numpy(c['gk'].astype(np.float64)))
    named = dict(net.named_parameters())
    for k in gq.PARAM_NAMES:
        t = named[k].grad.numpy()
        d = np.abs(t - c['G'][k]).max()
        scale = np.abs(t).max()
        print('%s %s: |float64 - torch double| = %.3e of max |g| %.3e' % (name, k, d, scale))
        assert scale > 0 and d <= 1e-9 * scale, k


def _adam_inputs(count, seed):
    rng = np.random.RandomState(seed)
    w = rng.standard_normal(count).astype(F)
    g = (0.1 * rng.standard_normal(count)).astype(F)
    m = (0.05 * rng.standard_normal(count)).astype(F)
    v = (0.01 * rng.uniform(size=count)).astype(F)
    # g = 0 and v = 0 (each alone and together), and a fresh state
    g[0:6] = 0
    v[3:9] = 0
    m[6:12] = 0
    return w, g, m, v


@pytest.mark.parametrize('step', (1, 1000))
def test_adam_restatement_is_within_the_derived_bound_of_float64(step):
    consts = gth.adam_constants(step, lr=3e-3)
    w, g, m, v = _adam_inputs(4096, step)
    if step == 1:
        m[:] = 0; v[:] = 0
    w1, m1, v1 = gth.adam(w, g, m, v, consts)
    w64, bound = gth.adam64(w, g, m, v, consts)
    assert w1.dtype == F and np.isfinite(w1).all() and (bound > 0).all()
    ratio = np.abs(w1.astype(np.float64) - w64) / bound
    print('adam t = %d: largest |restatement - float64| / bound = %.3e' % (step, ratio.max()))
    assert (ratio <= 1.0).all()
    # g = 0 with m = v = 0 changes nothing, bit for bit
    z = np.zeros(8, F)
    w2, m2, v2 = gth.adam(w[:8], z, z, z, consts)
    assert np.array_equal(_bits(w2), _bits(w[:8])) and not m2.any() and not v2.any()
    # the moments themselves
    b1, b2 = float(consts[1]), float(consts[2])
    assert np.allclose(m1, b1 * m.astype(np.float64) + (1 - b1) * g, rtol=4e-7, atol=0)
    assert np.allclose(v1, b2 * v.astype(np.float64) + (1 - b2) * g.astype(np.float64) ** 2, rtol=4e-7, atol=0)


@pytest.mark.parametrize('step', (1, 1000))
def test_adam_step_is_within_twice_the_bound_of_torch(step):
    """torch.optim.Adam with the same float32 betas (as Python floats), its state set to (step - 1, m, v)"""
    import torch
    lr, eps = 3e-3, 1e-8
    consts = gth.adam_constants(step, lr=lr, eps=eps)
    w, g, m, v = _adam_inputs(4096, 10 + step)
    if step == 1:
        m[:] = 0; v[:] = 0
    p = torch.nn.Parameter(torch.from_numpy(w.copy()))
    opt = torch.optim.Adam([p], lr=lr, betas=(float(consts[1]), float(consts[2])), eps=eps)
    if step > 1:
        opt.state[p] = {'step': torch.tensor(float(step - 1)), 'exp_avg': torch.from_numpy(m.copy()), 'exp_avg_sq': torch.from_numpy(v.copy())}
    p.grad = torch.from_numpy(g.copy())
    opt.step()
    w1, _, _ = gth.adam(w, g, m, v, consts)
    _, bound = gth.adam64(w, g, m, v, consts)
    ratio = np.abs(p.detach().numpy().astype(np.float64) - w1.astype(np.float64)) / (2.0 * bound)
    print('adam t = %d: largest |torch - restatement| / 2 bound = %.3e' % (step, ratio.max()))
    assert (ratio <= 1.0).all()
    assert int(opt.state[p]['step']) == step


@pytest.mark.parametrize('name', sorted(MODELS))
def test_from_blob_round_trips_bit_for_bit(name):
    m = _model(name, seed=5)
    r = GraspQualityModel.from_blob(m.blob(), m.norm, **m.sizes)
    assert r.sizes == m.sizes
    assert all(np.array_equal(_bits(r.params[k]), _bits(m.params[k])) and r.params[k].shape == m.params[k].shape for k in gq.PARAM_NAMES)
    assert all(np.array_equal(_bits(r.norm[k]), _bits(m.norm[k])) for k in gq.NORM_NAMES)
    assert np.array_equal(_bits(r.blob()), _bits(m.blob()))
    # grad_blob is blob()'s layout
    assert np.array_equal(_bits(gth.grad_blob(m.params)), _bits(m.blob()))
    with pytest.raises(ValueError):
        GraspQualityModel.from_blob(m.blob()[:-1], m.norm, **m.sizes)


def test_structs_and_workspace_match_the_c_side(tmp_path):
    import subprocess
    T = abi.rv_adam_params
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "rovat.h"\nint main(){printf("%zu %zu %zu %zu %d\\n", '
           'sizeof(rv_adam_params), offsetof(rv_adam_params, eps), offsetof(rv_adam_params, corr2), '
           'offsetof(rv_adam_params, reserved), RV_GQ_MAX_BATCH);return 0;}\n')
    (tmp_path / 't.c').write_text(src)
    subprocess.run(['gcc', '-I', os.path.join(HERE, '..', 'include'), str(tmp_path / 't.c'), '-o', str(tmp_path / 't')], check=True)
    out = subprocess.run([str(tmp_path / 't')], capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out] == [C.sizeof(T), T.eps.offset, T.corr2.offset, T.reserved.offset, abi.RV_GQ_MAX_BATCH]
    assert C.sizeof(T) == 32
    for name in ('rv_grasp_quality_train_workspace_floats', 'rv_grasp_quality_forward_train', 'rv_grasp_quality_backward', 'rv_adam_step'):
        assert name in lib.SYMBOLS and name in abi.GRASP_TRAIN_API
    floats = lib.load().rv_grasp_quality_train_workspace_floats
    for name in MODELS:
        m = _model(name)
        stride = gth.workspace_layout(**m.sizes)['stride']
        desc = m.descriptor()
        assert int(floats(C.byref(desc), 1)) == stride and int(floats(C.byref(desc), 70)) == 70 * stride
        assert int(floats(C.byref(desc), 0)) == -1 and int(floats(C.byref(desc), abi.RV_GQ_MAX_BATCH + 1)) == -1
    assert int(floats(None, 4)) == -1
    p = lib.adam_params(1000, lr=3e-3)
    c = gth.adam_constants(1000, lr=3e-3)
    assert [F(v) for v in (p.lr, p.beta1, p.beta2, p.eps, p.corr1, p.corr2)] == list(c)
    with pytest.raises(ValueError):
        lib.adam_params(0)
    with pytest.raises(ValueError):
        lib.adam_params(1, betas=(1.0, 0.999))
