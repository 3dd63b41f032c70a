"""The training step of the grasp-quality network on the MI355X: k_gq_train_forward,
k_gq_train_backward_sample, k_gq_train_backward_weights and k_adam_step compared bit for bit with tests/grasp_train_host.py
(their float32 NumPy restatement) -- logits, the workspace's activations, the per-sample parts and every gradient entry --
for the tiny, an 8 x 12 and the default model at batch sizes around a workgroup's 8 samples; the forward logits against
rv_grasp_quality's; Adam; three trainer steps; guard words, refusals, the world's state; and a training run that learns."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import grasp_quality_host as gqh
import grasp_train_host as gth
from robovat_amd import abi, configs, lib, scenes
from robovat_amd.perception import grasp_quality as gq
from robovat_amd.perception import grasp_quality_trainer
from robovat_amd.perception.grasp_quality import GraspQualityModel

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
F = np.float32
POISON = -7.0
NORM = dict(im_mean=0.45, im_inv_std=3.7, z_mean=0.55, z_inv_std=19.0)
MODELS = {
    'tiny': dict(gq.TINY_SIZES),
    '8x12': dict(height=8, width=12, c1=4, c2=8, f1=8, f2=4, p=4),
    'default': dict(gq.DEFAULT_SIZES),
}
# m = 1, 5, one more than a workgroup's 8 samples, and 70 (nine workgroups forward, the last with 6 samples; 70 backward)
CASES = [('tiny', m) for m in (1, 5, 9, 70)] + [('8x12', m) for m in (1, 5, 9, 70)] + [('default', 3)]
N_ENVS, K_ROWS = 5, 14      # N K = 70: the rows of the largest case as rv_grasp_quality takes them


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _differ(got, want):
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    assert got.shape == want.shape, (got.shape, want.shape)
    return int((_bits(got) != _bits(want)).sum())


@pytest.fixture(scope='module')
def world():
    """rv_grasp_quality_forward_train and the others take the device and the stream from it and nothing else"""
    scene, names = scenes.make_scene()
    cfg = configs.make_rv_config(env_cfg=configs.push_env_config(TASK_NAME='crossing', LAYOUT_ID=0), n_envs=N_ENVS,
                                 shape_names=names, seed=3)
    w = lib.World(cfg, scene, device=0)
    yield w
    w.close()


def _crafted_model(name):
    """a seeded model whose conv1 channels 0 .. 2 are made to hit the corners of the arithmetic: channel 0 copies the
    normalised image (equal pixels are equal maxima of a pool window), channel 1 is "a - a0" (exactly +0 where the pixel is
    0.6), channel 2 is "-a" with a -0 bias (-0 where the pixel is im_mean)"""
    m = GraspQualityModel.random_init(11, norm=NORM, **MODELS[name])
    q = m.params
    a0 = ((F(0.6) - F(NORM['im_mean'])).astype(F) * F(NORM['im_inv_std'])).astype(F)
    q['conv1.weight'][0:3] = 0
    q['conv1.weight'][0, 0, 2, 2] = 1; q['conv1.bias'][0] = 0
    q['conv1.weight'][1, 0, 2, 2] = 1; q['conv1.bias'][1] = -a0
    q['conv1.weight'][2, 0, 2, 2] = -1; q['conv1.bias'][2] = F(-0.0)
    return m


_REFERENCE = {}


def _reference(name, m):
    """(model, images, depths, dlogits, restatement logits, acts, gradients, per-sample parts) for the first ``m`` rows of
    the model's inputs, computed once per (model, m): the batch gradients are chains over all of a batch's rows"""
    if (name, m) not in _REFERENCE:
        model = _crafted_model(name)
        h, w = model.sizes['height'], model.sizes['width']
        x, z = gqh.sample_inputs(5, 70, h, w)              # a quarter of the pixels exactly 0
        x[0] = F(0.7)                                      # every pool window of channel 0: four equal positive values
        x[0, 1::3, 2::3] = F(0.6)                          # channel 1 cancels to +0 here
        x[0, 2::3, 0::3] = F(NORM['im_mean'])              # channel 2 is -0 here
        x[1] = 0                                           # an all-zero image (a crop outside the image)
        x[4, :, : w // 2] = F(0.6)
        g = np.random.RandomState(9).standard_normal(70).astype(F)
        g[2::4] = 0                                        # zeros and both signs
        assert (g > 0).any() and (g < 0).any() and g[0] != 0
        x, z, g = x[:m], z[:m], g[:m]
        logits, acts = gth.forward_train(model.params, model.norm, x, z)
        grads, parts = gth.backward(model.params, acts, g, parts=True)
        _REFERENCE[name, m] = (model, x, z, g, logits, acts, grads, parts)
    return _REFERENCE[name, m]


def _dev(world, a):
    return world.torch.as_tensor(np.ascontiguousarray(a), device=world.device)


@pytest.mark.parametrize('name,m', CASES)
def test_kernels_equal_the_host_restatement(world, name, m):
    t = world.torch
    model, x, z, g, want_logits, acts, grads, parts = _reference(name, m)
    # what row 0 was made for is there: window (0, 0) of channel 0 has four equal positive values and chose the first
    assert acts['i1'][0, 0, 0, 0] == 0 and acts['c1'][0, 0, 0, 0] > 0 and (acts['i1'][0, 0] > 0).any()
    assert np.isfinite(want_logits).all()
    blob = _dev(world, model.blob())
    xd, zd, gd = _dev(world, x), _dev(world, z), _dev(world, g)
    T = gth.workspace_layout(**model.sizes)
    count = model.weight_count()
    for lead in (4, 1):      # outputs 16-byte aligned and 4-byte aligned only, guard words around them
        lbuf = t.full((lead + m + 4,), POISON, dtype=t.float32, device=world.device)
        gbuf = t.full((lead + count + 4,), POISON, dtype=t.float32, device=world.device)
        wbuf = t.full((lead + m * T['stride'] + 4,), POISON, dtype=t.float32, device=world.device)
        lout, gout, ws = lbuf[lead:lead + m], gbuf[lead:lead + count], wbuf[lead:lead + m * T['stride']]
        assert (lout.data_ptr() % 16 == 0) == (lead == 4)
        got, ws2 = world.grasp_quality_forward_train(model, blob, xd, zd, workspace=ws, out=lout)
        assert got is lout and ws2 is ws
        d = _differ(got.cpu().numpy(), want_logits)
        print('%s m = %d lead %d: %d of %d logits differ' % (name, m, lead, d, m))
        assert d == 0
        rows = ws.cpu().numpy().reshape(m, T['stride'])
        for off, want in gth.workspace_rows(acts, T):
            assert _differ(rows[:, off:off + want.shape[1]], want) == 0, off
        grad = world.grasp_quality_backward(model, blob, xd, zd, gd, ws, out=gout)
        assert grad is gout
        rows = ws.cpu().numpy().reshape(m, T['stride'])
        for key in ('dz2', 'dzc', 's2', 's2b', 's1', 's1b'):
            want = parts[key]
            assert _differ(rows[:, T[key]:T[key] + want.shape[1]], want) == 0, key
        assert _differ(rows[:, T['g']], g) == 0
        for off, want in gth.workspace_rows(acts, T):      # the backward pass leaves the activations as they were
            assert _differ(rows[:, off:off + want.shape[1]], want) == 0, off
        got = gth.grad_blob(grads)
        d = _bits(grad.cpu().numpy()) != _bits(got)
        print('%s m = %d lead %d: %d of %d gradient entries differ' % (name, m, lead, int(d.sum()), count))
        assert not d.any(), np.flatnonzero(d)[:10]
        for buf, n in ((lbuf, m), (gbuf, count), (wbuf, m * T['stride'])):
            assert bool((buf[:lead] == POISON).all()) and bool((buf[lead + n:] == POISON).all())
    assert np.abs(gth.grad_blob(grads)).max() > 0


@pytest.mark.parametrize('name', ['tiny', 'default'])
def test_forward_train_logits_are_grasp_quality_logits(world, name):
    k = K_ROWS if name == 'tiny' else 1
    rows = N_ENVS * k
    model, x, z = _reference(name, 70 if name == 'tiny' else 3)[:3]
    if name == 'default':
        x2, z2 = gqh.sample_inputs(6, rows, 32, 32)
        x, z = np.concatenate([x, x2])[:rows], np.concatenate([z, z2])[:rows]
    h, w = model.sizes['height'], model.sizes['width']
    a = world.grasp_quality(x.reshape(N_ENVS, k, h, w), z.reshape(N_ENVS, k), model).cpu().numpy().reshape(-1)
    b, _ = world.grasp_quality_forward_train(model, _dev(world, model.blob()), _dev(world, x), _dev(world, z))
    assert _differ(b.cpu().numpy(), a) == 0 and len(set(a.tolist())) > 1


def _adam_case(count, step):
    rng = np.random.RandomState(count % 1000 + step)
    w = rng.standard_normal(count).astype(F)
    g = (0.1 * rng.standard_normal(count)).astype(F)
    m = (0.05 * rng.standard_normal(count)).astype(F)
    v = (0.01 * rng.uniform(size=count)).astype(F)
    if step == 1:
        m[:] = 0; v[:] = 0
    g[::7] = 0
    v[::5] = 0
    return w, g, m, v


@pytest.mark.parametrize('step', (1, 1000))
def test_adam_step_equals_the_host_restatement(world, step):
    t = world.torch
    counts = [1, 63, 65] + [GraspQualityModel.random_init(0, **MODELS[n]).weight_count() for n in sorted(MODELS)]
    consts = gth.adam_constants(step, lr=3e-3)
    for count in counts:
        w, g, m, v = _adam_case(count, step)
        w1, m1, v1 = gth.adam(w, g, m, v, consts)
        for lead in (4, 1):
            bufs = [t.full((lead + count + 4,), POISON, dtype=t.float32, device=world.device) for _ in range(4)]
            views = [b[lead:lead + count] for b in bufs]
            for view, a in zip(views, (w, g, m, v)):
                view.copy_(_dev(world, a))
            assert world.adam_step(views[0], views[1], views[2], views[3], step, lr=3e-3) is views[0]
            for view, want, what in zip(views, (w1, g, m1, v1), 'wgmv'):
                assert _differ(view.cpu().numpy(), want) == 0, (count, what)
            for b in bufs:
                assert bool((b[:lead] == POISON).all()) and bool((b[lead + count:] == POISON).all())


def test_three_trainer_steps_equal_the_restatement_on_the_host(world, monkeypatch):
    model = GraspQualityModel.random_init(4, norm=NORM, **MODELS['tiny'])
    x, z = gqh.sample_inputs(8, 3 * 12, 8, 8)
    y = (np.random.RandomState(3).uniform(size=len(x)) < 0.5).astype(F)
    seen = []
    real = grasp_quality_trainer.bce_with_logits

    def recording(torch, logits, labels, sample_weights=None):
        loss, d = real(torch, logits, labels, sample_weights)
        seen.append((logits.clone(), d.clone()))
        return loss, d
    monkeypatch.setattr(grasp_quality_trainer, 'bce_with_logits', recording)
    trainer = grasp_quality_trainer.GraspQualityTrainer(world, model, lr=3e-3)
    losses = [trainer.step(x[12 * i:12 * i + 12], z[12 * i:12 * i + 12], y[12 * i:12 * i + 12]) for i in range(3)]
    assert all(l.dim() == 0 and l.device == world.device for l in losses) and trainer.steps == 3
    # the host: the same three steps, the derivative of the loss taken from the device (no exponential is restated)
    cur = model
    blob, m, v = model.blob(), np.zeros(model.weight_count(), F), np.zeros(model.weight_count(), F)
    for i in range(3):
        xs, zs = x[12 * i:12 * i + 12], z[12 * i:12 * i + 12]
        logits, acts = gth.forward_train(cur.params, cur.norm, xs, zs)
        assert _differ(seen[i][0].cpu().numpy(), logits) == 0
        grads = gth.backward(cur.params, acts, seen[i][1].cpu().numpy())
        blob, m, v = gth.adam(blob, gth.grad_blob(grads), m, v, gth.adam_constants(i + 1, lr=3e-3))
        cur = GraspQualityModel.from_blob(blob, model.norm, **model.sizes)
    assert _differ(trainer.blob.cpu().numpy(), blob) == 0
    assert _differ(trainer.m.cpu().numpy(), m) == 0 and _differ(trainer.v.cpu().numpy(), v) == 0
    assert _differ(trainer.model().blob(), blob) == 0 and _differ(model.blob(), blob) > 0
    # a weighted step runs and is another step
    before = trainer.blob.clone()
    trainer.step(x[:12], z[:12], y[:12], sample_weights=np.linspace(0.5, 2.0, 12).astype(F))
    assert not bool((trainer.blob == before).all())
    with pytest.raises(ValueError):
        trainer.load_data(np.where(np.arange(64).reshape(1, 8, 8) == 10, np.nan, x[:1]), z[:1], y[:1])
    with pytest.raises(ValueError):
        trainer.load_data(x[:2], np.array([0.5, np.inf], F), y[:2])


def test_refusals_leave_the_outputs_untouched_and_the_world_as_it_was(world):
    t = world.torch
    model, x, z, g = _reference('tiny', 5)[:4]
    m = 5
    count = model.weight_count()
    T = gth.workspace_layout(**model.sizes)
    before = world.save_state().blocks.cpu().numpy().tobytes()
    pad = lambda a: _dev(world, np.concatenate([np.ravel(a), np.zeros(4, F)]))
    images, depths, dl, weights = pad(x), pad(z), pad(g), pad(model.blob())
    outs = {k: t.full((n + 8,), POISON, dtype=t.float32, device=world.device)
            for k, n in (('logits', m), ('grad', count), ('ws', m * T['stride']), ('w', count), ('m', count), ('v', count))}
    ptr = lambda v, off=0: None if v is None else C.c_void_p(v.data_ptr() + off)

    def untouched(what):
        world.synchronize()
        for k, v in outs.items():
            assert bool((v == POISON).all()), (what, k)

    def fwd(desc, wts=weights, img=images, dep=depths, mm=m, ws=outs['ws'], out=outs['logits'], off=(0,) * 5, what=''):
        rc = world.lib.rv_grasp_quality_forward_train(world.h, None if desc is None else C.byref(desc), ptr(wts, off[0]), ptr(img, off[1]),
                                                      ptr(dep, off[2]), mm, ptr(ws, off[3]), ptr(out, off[4]))
        assert rc == abi.RV_ERR_VALUE and what.encode() in world.lib.rv_last_error(), ('forward', what, rc)
        untouched(what)

    def bwd(desc, wts=weights, img=images, dep=depths, dlg=dl, mm=m, ws=outs['ws'], out=outs['grad'], off=(0,) * 6, what=''):
        rc = world.lib.rv_grasp_quality_backward(world.h, None if desc is None else C.byref(desc), ptr(wts, off[0]), ptr(img, off[1]),
                                                 ptr(dep, off[2]), ptr(dlg, off[3]), mm, ptr(ws, off[4]), ptr(out, off[5]))
        assert rc == abi.RV_ERR_VALUE and what.encode() in world.lib.rv_last_error(), ('backward', what, rc)
        untouched(what)

    def adam(p, n=count, w=outs['w'], gr=weights, mo=outs['m'], v=outs['v'], off=(0,) * 4, what=''):
        rc = world.lib.rv_adam_step(world.h, None if p is None else C.byref(p), n, ptr(w, off[0]), ptr(gr, off[1]), ptr(mo, off[2]), ptr(v, off[3]))
        assert rc == abi.RV_ERR_VALUE and what.encode() in world.lib.rv_last_error(), ('adam', what, rc)
        untouched(what)

    ok = model.descriptor()
    fwd(None, what='null model'); bwd(None, what='null model'); adam(None, what='null params')
    for key in ('wts', 'img', 'dep', 'ws', 'out'):
        fwd(ok, what='null buffer', **{key: None})
    for key in ('wts', 'img', 'dep', 'dlg', 'ws', 'out'):
        bwd(ok, what='null buffer', **{key: None})
    for byte in (1, 2):
        for i in range(5):
            fwd(ok, off=tuple(byte if j == i else 0 for j in range(5)), what='4-byte aligned')
        for i in range(6):
            bwd(ok, off=tuple(byte if j == i else 0 for j in range(6)), what='4-byte aligned')
        for i in range(4):
            adam(lib.adam_params(1), off=tuple(byte if j == i else 0 for j in range(4)), what='4-byte aligned')
    good = dict(gq.TINY_SIZES)
    for field, v in (('height', 4), ('width', 9), ('c1', 6), ('c2', abi.RV_GQ_MAX_CHANNELS + 4), ('f1', 0), ('f2', 6), ('p', 2), ('reserved', 1)):
        d = abi.rv_grasp_quality_model(im_inv_std=1, z_inv_std=1, **dict(good, **{field: v}))
        fwd(d, what='outside its range'); bwd(d, what='outside its range')
    for field in gq.NORM_NAMES:
        for v in (float('nan'), float('inf')):
            d = abi.rv_grasp_quality_model(**dict(dict(good, im_inv_std=1, z_inv_std=1), **{field: v}))
            fwd(d, what='not finite'); bwd(d, what='not finite')
    for mm in (0, -1, abi.RV_GQ_MAX_BATCH + 1):
        fwd(ok, mm=mm, what='m outside'); bwd(ok, mm=mm, what='m outside')
    # d_grad on top of an input or of the workspace; the forward pass's outputs on top of one another or of the weights
    for key, buf in (('wts', outs['grad']), ('img', outs['grad']), ('dep', outs['grad']), ('dlg', outs['grad']), ('ws', outs['grad'])):
        bwd(ok, what='must not overlap', **{key: buf})
    fwd(ok, ws=outs['ws'], out=outs['ws'], what='must not overlap')
    fwd(ok, wts=outs['ws'], what='must not overlap')
    for n in (0, -3):
        adam(lib.adam_params(1), n=n, what='count < 1')
    for field in ('lr', 'beta1', 'beta2', 'eps', 'corr1', 'corr2'):
        for v in (float('nan'), float('inf')):
            p = lib.adam_params(2)
            setattr(p, field, v)
            adam(p, what='not finite')
    for field in ('beta1', 'beta2'):
        for v in (1.0, -0.5, 1.5):
            p = lib.adam_params(2)
            setattr(p, field, v)
            adam(p, what='outside [0, 1)')
    p = lib.adam_params(2)
    p.reserved[1] = 1
    adam(p, what='reserved')
    adam(lib.adam_params(2), mo=outs['w'], what='must not overlap')
    adam(lib.adam_params(2), gr=outs['v'], what='must not overlap')
    # the binding raises ValueError for them, and checks the shapes itself
    blob = weights[:count]
    with pytest.raises(ValueError):
        world.grasp_quality_forward_train(model, blob, np.zeros((abi.RV_GQ_MAX_BATCH + 1, 8, 8), F), np.zeros(abi.RV_GQ_MAX_BATCH + 1, F))
    with pytest.raises(ValueError):
        world.grasp_quality_forward_train(model, blob, np.zeros((3, 8, 12), F), np.zeros(3, F))
    with pytest.raises(ValueError):
        world.grasp_quality_forward_train(model, blob[:-1], np.zeros((3, 8, 8), F), np.zeros(3, F))
    with pytest.raises(ValueError):
        world.grasp_quality_backward(model, blob, x, z, dl[:m], outs['ws'][:7])
    with pytest.raises(ValueError):
        world.adam_step(outs['w'][:count], outs['grad'][:count - 1], outs['m'][:count], outs['v'][:count], 1)
    untouched('bindings')
    # a real step, then: no env was read or written
    logits, ws = world.grasp_quality_forward_train(model, blob, x, z)
    world.grasp_quality_backward(model, blob, x, z, dl[:m], ws)
    world.synchronize()
    assert world.save_state().blocks.cpu().numpy().tobytes() == before


def _train_tool():
    spec = importlib.util.spec_from_file_location('train_grasp_quality', os.path.join(HERE, '..', 'tools', 'train_grasp_quality.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_it_learns(world):
    """the synthetic 8 x 8 set and recipe of tests/test_grasp_quality_host.py's smoke run, through backend='hip'"""
    tool = _train_tool()
    rng = np.random.RandomState(0)
    M = 512
    x = (0.6 + 0.05 * rng.standard_normal((M, 8, 8))).astype(F)
    z = (0.6 + 0.05 * rng.standard_normal(M)).astype(F)
    centre = x[:, 3:5, 3:5].mean(axis=(1, 2))
    y = (centre - z > 0).astype(F)
    model, history = tool.train(x, z, y, epochs=12, batch=32, lr=3e-3, seed=0, backend='hip', world=world, c1=4, c2=4, f1=8, f2=8, p=4)
    assert model.sizes['height'] == 8 and model.sizes['width'] == 8 and len(history) == 12
    q = float(y.mean())
    constant = -(q * np.log(q) + (1 - q) * np.log(1 - q))
    print('hip training: train loss %.4f -> %.4f, held-out loss %.4f, best constant %.4f, held-out accuracy %.3f'
          % (history[0]['train_loss'], history[-1]['train_loss'], history[-1]['holdout_loss'], constant, history[-1]['holdout_accuracy']))
    assert history[-1]['train_loss'] < history[0]['train_loss']
    assert history[-1]['train_loss'] < constant
    # the run is deterministic bit for bit
    again, _ = tool.train(x, z, y, epochs=2, batch=32, lr=3e-3, seed=0, backend='hip', world=world, c1=4, c2=4, f1=8, f2=8, p=4)
    once, _ = tool.train(x, z, y, epochs=2, batch=32, lr=3e-3, seed=0, backend='hip', world=world, c1=4, c2=4, f1=8, f2=8, p=4)
    assert _differ(again.blob(), once.blob()) == 0
