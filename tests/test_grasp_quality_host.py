"""The grasp-quality network without a GPU: tests/grasp_quality_host.py -- the float32 restatement of
csrc/rv_dev_grasp_quality.h -- against a float64 evaluation with a derived error bound B (its docstring), the training-side
torch module against the restatement within 2 B, the blob and the descriptor against the C side, hand-checkable networks,
the round trips, and a training smoke run of tools/train_grasp_quality.py."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import grasp_quality_host as gqh
from robovat_amd import abi, lib
from robovat_amd.perception import grasp_quality as gq
from robovat_amd.perception.grasp_quality import GraspQualityModel

HERE = os.path.dirname(os.path.abspath(__file__))
F = np.float32
NORM = dict(im_mean=0.45, im_inv_std=3.7, z_mean=0.55, z_inv_std=19.0)
MODELS = {
    'default': dict(gq.DEFAULT_SIZES),
    'tiny': dict(gq.TINY_SIZES),
    '8x12': dict(height=8, width=12, c1=8, c2=12, f1=20, f2=12, p=4),
}
COUNT = {'default': 6, 'tiny': 40, '8x12': 24}


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _model(name, seed=1):
    return GraspQualityModel.random_init(seed, norm=NORM, **MODELS[name])


@pytest.fixture(scope='module')
def evaluated():
    """name -> (model, images, depths, restatement logits, float64 logits, B), computed once"""
    out = {}
    for name in MODELS:
        m = _model(name)
        x, z = gqh.sample_inputs(7, COUNT[name], m.sizes['height'], m.sizes['width'])
        y64, B = gqh.forward64(m.params, m.norm, x, z)
        out[name] = (m, x, z, gqh.forward(m.params, m.norm, x, z), y64, B)
    return out


@pytest.mark.parametrize('name', sorted(MODELS))
def test_restatement_is_within_the_derived_bound_of_float64(evaluated, name):
    m, x, z, y, y64, B = evaluated[name]
    assert y.dtype == F and y.shape == (COUNT[name],) and np.isfinite(y).all() and (B > 0).all()
    ratio = np.abs(y.astype(np.float64) - y64) / B
    print('%s: largest |restatement - float64| / B = %.3e (B up to %.3e, |logit| up to %.3f)' % (name, ratio.max(), B.max(), np.abs(y64).max()))
    assert (ratio <= 1.0).all()


@pytest.mark.parametrize('name', sorted(MODELS))
def test_torch_module_is_within_twice_the_bound_of_the_restatement(evaluated, name):
    import torch
    m, x, z, y, y64, B = evaluated[name]
    net = m.torch_module()
    with torch.no_grad():
        t = net(torch.from_numpy(x), torch.from_numpy(z)).numpy()
    assert t.dtype == F and t.shape == y.shape
    ratio = np.abs(t.astype(np.float64) - y.astype(np.float64)) / (2.0 * B)
    print('%s: largest |torch - restatement| / 2B = %.3e' % (name, ratio.max()))
    assert (ratio <= 1.0).all()
    # the weights have no symmetry: a transposed conv tap or another flatten order is far outside the bound
    bad = dict(m.params)
    bad['conv2.weight'] = np.ascontiguousarray(m.params['conv2.weight'].transpose(0, 1, 3, 2))
    yb = gqh.forward(bad, m.norm, x[:2], z[:2])
    assert (np.abs(yb.astype(np.float64) - y64[:2]) > 2.0 * B[:2]).any()


@pytest.mark.parametrize('name', sorted(MODELS))
def test_blob_has_the_length_the_library_counts(name):
    m = _model(name)
    desc = m.descriptor()
    count = int(lib.load().rv_grasp_quality_weight_count(C.byref(desc)))
    assert count == m.blob().size == m.weight_count() and m.blob().dtype == F
    if name == 'default':
        assert count == 73617
    # the blob is K-major for conv2 and the fc layers: element [k][n] of the blob is weight[n][k]
    s, b = m.sizes, m.blob()
    o = 26 * s['c1']
    w2 = b[o:o + 9 * s['c1'] * s['c2']].reshape(9 * s['c1'], s['c2'])
    assert w2[1 * 9 + 2 * 3 + 1, 3] == m.params['conv2.weight'][3, 1, 2, 1]
    o += w2.size + s['c2']
    k1 = s['c2'] * (s['height'] // 4) * (s['width'] // 4)
    assert b[o + 5 * s['f1'] + 2] == m.params['fc1.weight'][2, 5]
    assert b[-1] == m.params['out.bias'][0] and b[0] == m.params['conv1.weight'][0, 0, 0, 0]
    assert o + k1 * s['f1'] < b.size


def test_refused_descriptors_count_minus_one():
    count = lib.load().rv_grasp_quality_weight_count
    assert int(count(None)) == -1
    good = dict(gq.DEFAULT_SIZES)
    for field, values in (('height', (4, 36, 30)), ('width', (0, 64, 10)), ('c1', (0, 20, 6)), ('c2', (-4, 20, 15)),
                          ('f1', (0, 132, 7)), ('f2', (0, 132, 63)), ('p', (0, 36, 5))):
        for v in values:
            d = abi.rv_grasp_quality_model(im_inv_std=1, z_inv_std=1, **dict(good, **{field: v}))
            assert int(count(C.byref(d))) == -1, (field, v)
            with pytest.raises(ValueError):
                GraspQualityModel.random_init(0, **dict(good, **{field: v}))
    d = abi.rv_grasp_quality_model(reserved=1, **good)
    assert int(count(C.byref(d))) == -1
    # the limits themselves are models
    big = dict(height=abi.RV_GQ_MAX_SIDE, width=abi.RV_GQ_MAX_SIDE, c1=abi.RV_GQ_MAX_CHANNELS, c2=abi.RV_GQ_MAX_CHANNELS,
               f1=abi.RV_GQ_MAX_FEATURES, f2=abi.RV_GQ_MAX_FEATURES, p=abi.RV_GQ_MAX_POSE)
    for sizes in (big, gq.TINY_SIZES):
        d = abi.rv_grasp_quality_model(**sizes)
        assert int(count(C.byref(d))) == sum(int(np.prod(s)) for s in gq.param_shapes(**sizes).values())


def test_model_struct_matches_the_c_layout(tmp_path):
    import subprocess
    T = abi.rv_grasp_quality_model
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "rovat.h"\nint main(){printf("%zu %zu %zu %zu %zu %d %d %d %d %d\\n", '
           'sizeof(rv_grasp_quality_model), offsetof(rv_grasp_quality_model, c1), offsetof(rv_grasp_quality_model, reserved), '
           'offsetof(rv_grasp_quality_model, im_mean), offsetof(rv_grasp_quality_model, z_inv_std), '
           'RV_GQ_MIN_SIDE, RV_GQ_MAX_SIDE, RV_GQ_MAX_CHANNELS, RV_GQ_MAX_FEATURES, RV_GQ_MAX_POSE);return 0;}\n')
    (tmp_path / 't.c').write_text(src)
    subprocess.run(['gcc', '-I', os.path.join(HERE, '..', 'include'), str(tmp_path / 't.c'), '-o', str(tmp_path / 't')], check=True)
    out = subprocess.run([str(tmp_path / 't')], capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out] == [C.sizeof(T), T.c1.offset, T.reserved.offset, T.im_mean.offset, T.z_inv_std.offset,
                                     abi.RV_GQ_MIN_SIDE, abi.RV_GQ_MAX_SIDE, abi.RV_GQ_MAX_CHANNELS, abi.RV_GQ_MAX_FEATURES,
                                     abi.RV_GQ_MAX_POSE]
    assert C.sizeof(T) == 48
    for name in ('rv_grasp_quality', 'rv_grasp_quality_weight_count'):
        assert name in lib.SYMBOLS and name in abi.GRASP_QUALITY_API


def _zero_model(**sizes):
    shapes = gq.param_shapes(**sizes)
    return GraspQualityModel({k: np.zeros(s, F) for k, s in shapes.items()}, NORM, **sizes)


def test_hand_checkable_networks():
    sizes = dict(height=8, width=12, c1=4, c2=4, f1=8, f2=4, p=4)
    x, z = gqh.sample_inputs(3, 5, 8, 12)
    # all zero: the last bias
    m = _zero_model(**sizes)
    m.params['out.bias'][0] = F(-1.75)
    assert np.array_equal(_bits(gqh.forward(m.params, m.norm, x, z)), _bits(np.full(5, -1.75, F)))
    # only the pose stream: logit = b + w_out relu(w2 relu(wp u + bp)) with u = (z - z_mean) z_inv_std, in closed form
    m = _zero_model(**sizes)
    m.params['pose.weight'][2, 0] = F(1.5); m.params['pose.bias'][2] = F(0.25)
    m.params['fc2.weight'][1, sizes['f1'] + 2] = F(2.0)
    m.params['out.weight'][0, 1] = F(-3.0); m.params['out.bias'][0] = F(0.5)
    u = ((z - F(NORM['z_mean'])) * F(NORM['z_inv_std'])).astype(F)
    p = np.maximum(gqh.fma(u, F(1.5), F(0.25)), 0)      # (2 p and -3 (2 p) + 0.5 are exact enough to write with fma too)
    want = gqh.fma(gqh.fma(p, F(2.0), F(0.0)), F(-3.0), F(0.5))
    got = gqh.forward(m.params, m.norm, x, z)
    assert np.array_equal(_bits(got), _bits(want)) and len(set(got.tolist())) > 1
    # and the images play no part
    assert np.array_equal(_bits(gqh.forward(m.params, m.norm, x[::-1], z)), _bits(want))
    # one unit conv1 tap reaching over the border: the padding is zero in the NORMALISED image.  Tap (0, 0) of a 5 x 5
    # kernel reads pixel (y - 2, x - 2); after pool2, c1[0][0][0] = max over y, x in {0, 1} = relu(0) = 0 (all four read the
    # padding), while c1[0][1][1] = max(relu(a[0..1][0..1])).  conv2's centre tap, fc1 reading one flat index and the head
    # carry that single value to the logit.
    m = _zero_model(**sizes)
    m.norm['im_mean'], m.norm['im_inv_std'] = F(0.25), F(2.0)
    m.params['conv1.weight'][0, 0, 0, 0] = F(1.0)
    m.params['conv2.weight'][0, 0, 1, 1] = F(1.0)
    m.params['fc2.weight'][0, 0] = F(1.0)
    m.params['out.weight'][0, 0] = F(1.0)
    img = np.full((1, 8, 12), 0.25, F)          # normalises to 0 everywhere ...
    img[0, 0:2, 0:2] = [[1.25, 0.75], [0.5, 0.0]]      # ... but here: 2, 1, 0.5, -0.5
    # c2[0] is [2][3] = pool2 of c1[0] [4][6]; c1[0][1][1] sits in c2[0][0][0]'s window, c1[0][0][0] (padding) too
    m.params['fc1.weight'][0, 0] = F(1.0)
    assert gqh.forward(m.params, m.norm, img, np.zeros(1, F))[0] == F(2.0)
    # a padding of the RAW image with zeros would normalise to (0 + 1) 2 = 2 at c1[0][0][0] and give the logit 2:
    m.norm['im_mean'] = F(-1.0)
    img2 = np.full((1, 8, 12), -1.0, F)  # normalises to 0: with zero padding of the normalised image the logit is 0
    assert gqh.forward(m.params, m.norm, img2, np.zeros(1, F))[0] == F(0.0)
    y64, B = gqh.forward64(m.params, m.norm, img2, np.zeros(1, F))
    assert y64[0] == 0.0


def test_save_load_and_module_round_trips_are_bit_equal(tmp_path):
    import torch
    m = _model('8x12', seed=4)
    path = str(tmp_path / 'model.npz')
    m.save(path)
    r = GraspQualityModel.load(path)
    assert r.sizes == m.sizes
    assert all(np.array_equal(_bits(r.norm[k]), _bits(m.norm[k])) for k in gq.NORM_NAMES)
    assert all(np.array_equal(_bits(r.params[k]), _bits(m.params[k])) for k in gq.PARAM_NAMES)
    assert np.array_equal(_bits(r.blob()), _bits(m.blob()))
    net = m.torch_module()
    assert isinstance(net, torch.nn.Module) and isinstance(net, gq.GraspQualityModule)
    assert sorted(k for k, _ in net.named_parameters()) == sorted(gq.PARAM_NAMES)
    b = GraspQualityModel.from_torch_module(net)
    assert b.sizes == m.sizes and np.array_equal(_bits(b.blob()), _bits(m.blob()))
    assert all(np.array_equal(_bits(b.norm[k]), _bits(m.norm[k])) for k in gq.NORM_NAMES)
    other = GraspQualityModel.from_torch_module(net, norm={'z_mean': 0.125})
    assert other.norm['z_mean'] == F(0.125) and other.norm['im_mean'] == m.norm['im_mean']
    # same seed, same model; another seed, another model
    assert np.array_equal(_bits(_model('8x12', seed=4).blob()), _bits(m.blob()))
    assert not np.array_equal(_bits(_model('8x12', seed=5).blob()), _bits(m.blob()))
    with pytest.raises(ValueError):
        GraspQualityModel(dict(m.params, **{'fc1.weight': m.params['fc1.weight'].T}), **m.sizes)
    with pytest.raises(TypeError):
        GraspQualityModel.random_init(0, depth=3)


def _train_tool():
    spec = importlib.util.spec_from_file_location('train_grasp_quality', os.path.join(HERE, '..', 'tools', 'train_grasp_quality.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_training_smoke_beats_the_best_constant_and_exports_what_it_trained():
    import torch
    tool = _train_tool()
    rng = np.random.RandomState(0)
    M = 512
    x = (0.6 + 0.05 * rng.standard_normal((M, 8, 8))).astype(F)
    z = (0.6 + 0.05 * rng.standard_normal(M)).astype(F)
    centre = x[:, 3:5, 3:5].mean(axis=(1, 2))
    y = (centre - z > 0).astype(F)
    assert 0.3 < y.mean() < 0.7
    torch.set_num_threads(1)
    model, history = tool.train(x, z, y, epochs=12, batch=32, lr=3e-3, seed=0, c1=4, c2=4, f1=8, f2=8, p=4)
    assert model.sizes['height'] == 8 and model.sizes['width'] == 8 and len(history) == 12
    # the best constant predictor of a set with positive rate q has cross-entropy H(q)
    q = float(y.mean())
    constant = -(q * np.log(q) + (1 - q) * np.log(1 - q))
    print('training smoke: train loss %.4f, held-out loss %.4f, best constant %.4f, held-out accuracy %.3f'
          % (history[-1]['train_loss'], history[-1]['holdout_loss'], constant, history[-1]['holdout_accuracy']))
    assert history[-1]['train_loss'] < constant and history[-1]['holdout_loss'] < constant
    # the exported model is the module: the restatement reproduces the module's logits within 2 B
    net = model.torch_module()
    with torch.no_grad():
        t = net(torch.from_numpy(x[:32]), torch.from_numpy(z[:32])).numpy()
    got = gqh.forward(model.params, model.norm, x[:32], z[:32])
    _, B = gqh.forward64(model.params, model.norm, x[:32], z[:32])
    assert (np.abs(t.astype(np.float64) - got.astype(np.float64)) <= 2.0 * B).all()
    n = tool.normalisation(x, z)
    assert abs(n['im_mean'] - x.mean()) < 1e-6 and abs(n['z_inv_std'] - 1.0 / z.astype(np.float64).std()) < 1e-6
