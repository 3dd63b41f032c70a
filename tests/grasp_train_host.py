"""NumPy restatement of csrc/rv_dev_grasp_train.h (rv_grasp_quality_forward_train, rv_grasp_quality_backward,
rv_adam_step), for the tests: float32, operation for operation, on top of the exact ``fma`` of tests/cem_host.py and of
tests/grasp_quality_host.py.  ``forward_train`` is that module's forward pass keeping what the workspace keeps;
``backward`` follows the header's chains: "fma chain of (a_k, b_k)" is acc = +0; acc = fma(a_k, b_k, acc), "sum chain" is
acc = +0; acc = acc + t_k; a term that does not pass (a pool window whose pooled value is not > 0, a tap that does not
land on a chosen position) is no term at all -- ``np.where(passes, fma(...), acc)``.  Gradients come back under torch's
parameter names and natural layouts; ``grad_blob`` puts them into the blob's layout.

``backward64`` is an independent float64 evaluation of the same gradients (dense unpooling, correlations and transposed
convolutions instead of chains over windows) on ``forward64_train``'s activations, and returns beside every gradient entry
a DERIVED bound on the error of the float32 chains.  Derivation, with u = 2^-24 and gamma_n = n u / (1 - n u) as in
tests/grasp_quality_host.py: a float32 chain of K terms a_i g_i, fused or not, from +0, whose inputs carry errors ea_i and
eg_i against the float64 values a_i and g_i, has

    |delta| <= gamma_(K+1) sum (|a_i| + ea_i)(|g_i| + eg_i) + sum (|a_i| eg_i + |g_i| ea_i + ea_i eg_i)

(the first term: the chain's own roundings on the inputs it saw; the second: what the inputs' errors do to the exact sum);
a sum chain of K terms t_i with errors e_i has |delta| <= gamma_K sum (|t_i| + e_i) + sum e_i.  Both hold PROVIDED the relu
and pool masks agree between the two precisions, so that the same terms are in the same chains; ``masks`` /
``masks_agree`` find the samples where they do.  K is taken at its largest (every window passing).  The activations'
errors are those of ``grasp_quality_host``'s forward bound; weights and dlogits are exact.

Adam.  ``adam`` restates k_adam_step; ``adam64`` evaluates the same update in float64 and bounds the float32 result.  The
float32 update has fourteen roundings: omb1 = fl(1 - beta1), t = fl(omb1 g), m' = fl(beta1 m + t) (one, fused);
omb2, fl(omb2 g), fl(. g), v' (fused); mh = fl(m' corr1), vh = fl(v' corr2), s = fl(sqrt(vh)), d = fl(s + eps),
n = fl(lr mh), q = fl(n / d), w' = fl(w - q).  With relative error u per rounding:
    em  = gamma_3 (|beta1 m| + |(1 - beta1) g|)            ev  = gamma_4 (beta2 v + (1 - beta2) g^2)
    emh = corr1 em (1 + u) + u |mh|                        evh = corr2 ev (1 + u) + u vh
    es  = evh / sqrt(vh) (0 where vh = 0: then evh = 0 too) + u (sqrt(vh) + that)
    ed  = es + u (d + es)                                  en  = lr emh (1 + u) + u |n|
    eq  = ((en + |q| ed) / (d - ed)) (1 + u) + u |q|       ew  = eq + u (|w'| + eq)
(|sqrt(a) - sqrt(b)| = |a - b| / (sqrt(a) + sqrt(b)) <= |a - b| / sqrt(b); the quotient's bound is the usual one for a
perturbed numerator and denominator, d - ed > 0 because d >= eps > 0).  Underflow is not modelled: the tests' values are
normal or exactly 0."""
import numpy as np

import grasp_quality_host as gqh
from cem_host import fma
from grasp_quality_host import F, U, gamma, relu

Z = F(0)


# ---------------------------------------------------------------------------------------------------------------------
# float32 forward, keeping the workspace

def pool2_idx(r):
    """(maximum, chosen position 0..3 = 2 row + column) of the 2 x 2 windows of the last two axes of ``r`` (after relu), in
    gq_pool's order: v00, then v01, v10, v11 each under a strict >"""
    m = r[..., 0::2, 0::2]
    s = np.zeros(m.shape, np.int32)
    for j, b in ((1, r[..., 0::2, 1::2]), (2, r[..., 1::2, 0::2]), (3, r[..., 1::2, 1::2])):
        t = b > m
        m = np.where(t, b, m)
        s = np.where(t, np.int32(j), s)
    return m, s


def normalise(norm, x, z):
    with np.errstate(invalid='ignore', over='ignore'):
        a = ((x - F(norm['im_mean'])).astype(F) * F(norm['im_inv_std'])).astype(F)
        u = ((z - F(norm['z_mean'])).astype(F) * F(norm['z_inv_std'])).astype(F)
    return a, u


def forward_train(params, norm, images, depths):
    """(logits float32 [S], acts): ``grasp_quality_host.forward``'s chains; ``acts`` holds c1 [S, C1, h/2, w/2], i1 (int32,
    the chosen positions), c2, i2, cat = f1 | p [S, F1 + P], f2 [S, F2], u [S] and a [S, h, w] the normalised image"""
    q = params
    x = np.ascontiguousarray(images, F)
    z = np.ascontiguousarray(depths, F).reshape(-1)
    S, h, w = x.shape
    a, u = normalise(norm, x, z)
    with np.errstate(invalid='ignore', over='ignore'):
        w1, b1 = q['conv1.weight'], q['conv1.bias']
        C1 = w1.shape[0]
        ap = np.zeros((S, h + 4, w + 4), F)
        ap[:, 2:-2, 2:-2] = a
        acc = np.broadcast_to(b1[None, :, None, None], (S, C1, h, w)).astype(F)
        acc = gqh._chain(acc, ((ap[:, None, ky:ky + h, kx:kx + w], w1[None, :, 0, ky, kx, None, None])
                               for ky in range(5) for kx in range(5)))
        c1, i1 = pool2_idx(relu(acc))
        w2, b2 = q['conv2.weight'], q['conv2.bias']
        C2 = w2.shape[0]
        H1, W1 = h // 2, w // 2
        cp = np.zeros((S, C1, H1 + 2, W1 + 2), F)
        cp[:, :, 1:-1, 1:-1] = c1
        acc = np.broadcast_to(b2[None, :, None, None], (S, C2, H1, W1)).astype(F)
        acc = gqh._chain(acc, ((cp[:, ci, None, ky:ky + H1, kx:kx + W1], w2[None, :, ci, ky, kx, None, None])
                               for ci in range(C1) for ky in range(3) for kx in range(3)))
        c2, i2 = pool2_idx(relu(acc))
        f1 = relu(gqh._fc(c2.reshape(S, -1), q['fc1.weight'], q['fc1.bias']))
        p = relu(gqh._fc(u[:, None], q['pose.weight'], q['pose.bias']))
        cat = np.concatenate([f1, p], axis=1)
        f2 = relu(gqh._fc(cat, q['fc2.weight'], q['fc2.bias']))
        logits = gqh._fc(f2, q['out.weight'], q['out.bias'])[:, 0]
    return logits.astype(F), dict(c1=c1, i1=i1, c2=c2, i2=i2, cat=cat, f2=f2, u=u, a=a)


def workspace_rows(acts, stride_info):
    """the floats the forward kernel writes into each sample's workspace row, as (offset, array [S, n]) pairs;
    ``stride_info``: ``workspace_layout`` of the model's sizes"""
    T = stride_info
    S = len(acts['u'])
    return [(T['c1'], acts['c1'].reshape(S, -1)), (T['i1'], acts['i1'].reshape(S, -1).astype(F)),
            (T['c2'], acts['c2'].reshape(S, -1)), (T['i2'], acts['i2'].reshape(S, -1).astype(F)),
            (T['cat'], acts['cat']), (T['f2'], acts['f2']), (T['u'], acts['u'][:, None])]


def workspace_layout(height, width, c1, c2, f1, f2, p):
    """gt_layout's offsets (floats) into a sample's row of the workspace"""
    n1 = (height // 2) * (width // 2)
    k1 = c2 * (height // 4) * (width // 4)
    T, at = {}, 0
    for name, n in (('c1', c1 * n1), ('i1', c1 * n1), ('c2', k1), ('i2', k1), ('cat', f1 + p), ('f2', f2), ('u', 1), ('g', 1),
                    ('dz2', f2), ('dzc', f1 + p), ('s2', 9 * c1 * c2), ('s2b', c2), ('s1', 25 * c1), ('s1b', c1)):
        T[name] = at
        at += n
    T['stride'] = at
    return T


# ---------------------------------------------------------------------------------------------------------------------
# float32 backward

def backward(params, acts, dlogits, route_v00=False, parts=False):
    """name -> gradient (float32, torch's natural layouts) of sum_b dlogits[b] logit[b].  ``route_v00``: a PLANTED ERROR for
    the tests -- every pool gradient goes to v00 instead of the chosen position.  ``parts``: also return the per-sample
    quantities (dz2, dzc, s2, s2b, s1, s1b) the kernel leaves in the workspace."""
    q = params
    g = np.ascontiguousarray(dlogits, F).reshape(-1)
    c1, c2, cat, f2, u, a = acts['c1'], acts['c2'], acts['cat'], acts['f2'], acts['u'], acts['a']
    i1, i2 = (np.zeros_like(acts['i1']), np.zeros_like(acts['i2'])) if route_v00 else (acts['i1'], acts['i2'])
    S, C1, H1, W1 = c1.shape
    C2, H2, W2 = c2.shape[1:]
    P2 = H2 * W2
    F1 = q['fc1.weight'].shape[0]
    F2 = q['fc2.weight'].shape[0]
    sidx = np.arange(S)
    with np.errstate(invalid='ignore', over='ignore'):
        # -- the head
        dz2 = np.where(f2 > 0, fma(g[:, None], q['out.weight'][0][None, :], Z), Z).astype(F)
        acc = np.zeros(cat.shape, F)
        for o in range(F2):
            acc = fma(dz2[:, o, None], q['fc2.weight'][o][None, :], acc)
        dzc = np.where(cat > 0, acc, Z).astype(F)
        c2f = c2.reshape(S, -1)
        acc = np.zeros(c2f.shape, F)
        for o in range(F1):
            acc = fma(dzc[:, o, None], q['fc1.weight'][o][None, :], acc)
        g2 = np.where(c2f > 0, acc, Z).astype(F).reshape(S, C2, P2)
        sel2 = np.where(c2f > 0, i2.reshape(S, -1), -1).reshape(S, C2, P2)
        # -- conv2's weights and bias, per sample
        cp = np.zeros((S, C1, H1 + 2, W1 + 2), F)
        cp[:, :, 1:-1, 1:-1] = c1
        s2 = np.zeros((S, C2, C1, 3, 3), F)
        s2b = np.zeros((S, C2), F)
        k3 = np.arange(3)
        for qi in range(P2):
            qy, qx = divmod(qi, W2)
            s = sel2[:, :, qi]
            ok = s >= 0
            sp = s & 3
            y, x = 2 * qy + (sp >> 1), 2 * qx + (sp & 1)                         # [S, C2]
            val = cp[sidx[:, None, None, None, None], np.arange(C1)[None, None, :, None, None],
                     y[:, :, None, None, None] + k3[None, None, None, :, None], x[:, :, None, None, None] + k3[None, None, None, None, :]]
            gq = g2[:, :, qi]
            s2 = np.where(ok[:, :, None, None, None], fma(gq[:, :, None, None, None], val, s2), s2)
            s2b = np.where(ok, (s2b + gq).astype(F), s2b)
        # -- the gradient at c1
        w2 = q['conv2.weight']
        acc = np.zeros((S, C1, H1, W1), F)
        ys, xs = np.arange(H1), np.arange(W1)
        for co in range(C2):
            for ky in range(3):
                for kx in range(3):
                    yo, xo = ys - ky + 1, xs - kx + 1
                    inb = ((yo >= 0) & (yo < H1))[:, None] & ((xo >= 0) & (xo < W1))[None, :]
                    yc, xc = np.clip(yo, 0, H1 - 1), np.clip(xo, 0, W1 - 1)
                    qidx = (yc >> 1)[:, None] * W2 + (xc >> 1)[None, :]              # [H1, W1]
                    pat = ((yc & 1) << 1)[:, None] | (xc & 1)[None, :]
                    hit = inb[None] & (sel2[:, co][:, qidx] == pat[None])            # [S, H1, W1]
                    gv = g2[:, co][:, qidx]
                    acc = np.where(hit[:, None], fma(gv[:, None], w2[co, :, ky, kx][None, :, None, None], acc), acc)
        g1 = np.where(c1 > 0, acc, Z).astype(F)
        # -- conv1's weights and bias, per sample
        h, w = a.shape[1:]
        ap = np.zeros((S, h + 4, w + 4), F)
        ap[:, 2:-2, 2:-2] = a
        s1 = np.zeros((S, C1, 5, 5), F)
        s1b = np.zeros((S, C1), F)
        k5 = np.arange(5)
        for qi in range(H1 * W1):
            qy, qx = divmod(qi, W1)
            ok = c1[:, :, qy, qx] > 0
            sp = i1[:, :, qy, qx]
            y, x = 2 * qy + (sp >> 1), 2 * qx + (sp & 1)
            val = ap[sidx[:, None, None, None], y[:, :, None, None] + k5[None, None, :, None], x[:, :, None, None] + k5[None, None, None, :]]
            gq = g1[:, :, qy, qx]
            s1 = np.where(ok[:, :, None, None], fma(gq[:, :, None, None], val, s1), s1)
            s1b = np.where(ok, (s1b + gq).astype(F), s1b)
        # -- over the batch, b ascending
        out = {}

        def fma_chain(dy, x):
            acc = np.zeros((dy.shape[1], x.shape[1]), F)
            for b in range(S):
                acc = fma(dy[b][:, None], x[b][None, :], acc)
            return acc

        def sum_chain(t):
            acc = np.zeros(t.shape[1:], F)
            for b in range(S):
                acc = (acc + t[b]).astype(F)
            return acc
        out['out.weight'] = fma_chain(g[:, None], f2)
        out['out.bias'] = sum_chain(g[:, None])
        out['fc2.weight'] = fma_chain(dz2, cat)
        out['fc2.bias'] = sum_chain(dz2)
        out['pose.weight'] = fma_chain(dzc[:, F1:], u[:, None])
        out['pose.bias'] = sum_chain(dzc[:, F1:])
        out['fc1.weight'] = fma_chain(dzc[:, :F1], c2f)
        out['fc1.bias'] = sum_chain(dzc[:, :F1])
        out['conv2.weight'] = sum_chain(s2)
        out['conv2.bias'] = sum_chain(s2b)
        out['conv1.weight'] = sum_chain(s1)[:, None]
        out['conv1.bias'] = sum_chain(s1b)
    out = {k: np.ascontiguousarray(v, F) for k, v in out.items()}
    if parts:
        # (s2 in the kernel's K-major order: [(ci 9 + ky 3 + kx)][co])
        return out, dict(g=g, dz2=dz2, dzc=dzc, s2=s2.transpose(0, 2, 3, 4, 1).reshape(S, -1), s2b=s2b, s1=s1.reshape(S, -1), s1b=s1b)
    return out


def grad_blob(grads):
    """the gradients in the blob's layout (``GraspQualityModel.blob``'s: conv2 and the fc weights K-major)"""
    c2, c1 = grads['conv2.weight'].shape[:2]
    parts = [grads['conv1.weight'].reshape(c1, 25), grads['conv1.bias'], grads['conv2.weight'].reshape(c2, 9 * c1).T,
             grads['conv2.bias'], grads['fc1.weight'].T, grads['fc1.bias'], grads['pose.weight'].reshape(-1), grads['pose.bias'],
             grads['fc2.weight'].T, grads['fc2.bias'], grads['out.weight'].reshape(-1), grads['out.bias']]
    return np.concatenate([np.ascontiguousarray(a, F).ravel() for a in parts])


# ---------------------------------------------------------------------------------------------------------------------
# float64 forward and backward with the running bound

def _pool64_idx(y, e):
    """relu + 2 x 2 maximum in float64 (ties to the first), the window's largest error, the chosen position"""
    r = np.maximum(y, 0)
    m, s = pool2_idx(r)
    ew = np.stack([e[..., 0::2, 0::2], e[..., 0::2, 1::2], e[..., 1::2, 0::2], e[..., 1::2, 1::2]]).max(axis=0)
    return m, ew, s


def forward64_train(params, norm, images, depths):
    """``grasp_quality_host.forward64`` keeping its activations: (logits, B, acts) with acts[name] = (value, error bound)
    for a, u, c1, c2, cat, f2 and the chosen positions i1, i2"""
    q = params
    x = np.asarray(images, F).astype(np.float64)
    z = np.asarray(depths, F).astype(np.float64).reshape(-1)
    a = (x - float(norm['im_mean'])) * float(norm['im_inv_std'])
    u = (z - float(norm['z_mean'])) * float(norm['z_inv_std'])
    ea, eu = gamma(2) * np.abs(a), gamma(2) * np.abs(u)
    y, e = gqh._layer64(a[:, None], ea[:, None], q['conv1.weight'], q['conv1.bias'], 25, conv=2)
    c1, e1, i1 = _pool64_idx(y, e)
    y, e = gqh._layer64(c1, e1, q['conv2.weight'], q['conv2.bias'], 9 * c1.shape[1], conv=1)
    c2, e2, i2 = _pool64_idx(y, e)
    S = len(x)
    y, e = gqh._layer64(c2.reshape(S, -1), e2.reshape(S, -1), q['fc1.weight'], q['fc1.bias'], q['fc1.weight'].shape[1])
    f1, ef1 = np.maximum(y, 0), e
    y, e = gqh._layer64(u[:, None], eu[:, None], q['pose.weight'], q['pose.bias'], 1)
    p, ep = np.maximum(y, 0), e
    cat, ecat = np.concatenate([f1, p], axis=1), np.concatenate([ef1, ep], axis=1)
    y, e = gqh._layer64(cat, ecat, q['fc2.weight'], q['fc2.bias'], cat.shape[1])
    f2, ef2 = np.maximum(y, 0), e
    y, e = gqh._layer64(f2, ef2, q['out.weight'], q['out.bias'], f2.shape[1])
    acts = dict(a=(a, ea), u=(u, eu), c1=(c1, e1), c2=(c2, e2), cat=(cat, ecat), f2=(f2, ef2), i1=i1, i2=i2)
    return y[:, 0], e[:, 0], acts


def masks(acts):
    """what decides which terms are in which chains: the relu signs and, where a window passes, its chosen position.
    ``acts`` of ``forward_train`` or of ``forward64_train``.  Returns one int array [S, n]"""
    def val(k):
        v = acts[k]
        return v[0] if isinstance(v, tuple) else v
    c1, c2, cat, f2 = val('c1'), val('c2'), val('cat'), val('f2')
    S = len(cat)
    parts = [np.where(c1 > 0, acts['i1'], -1).reshape(S, -1), np.where(c2 > 0, acts['i2'], -1).reshape(S, -1),
             (cat > 0).astype(np.int32), (f2 > 0).astype(np.int32)]
    return np.concatenate(parts, axis=1)


def masks_agree(acts32, acts64):
    """bool [S]: the samples whose float32 and float64 masks are the same"""
    return (masks(acts32) == masks(acts64)).all(axis=1)


def _unpool(g, sel, ok):
    """[S, C, H, W] -> [S, C, 2H, 2W]: g at the chosen position of the windows that pass, 0 elsewhere"""
    out = np.zeros(g.shape[:2] + (2 * g.shape[2], 2 * g.shape[3]))
    for j, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        out[..., dy::2, dx::2] = np.where(ok & (sel == j), g, 0.0)
    return out


def _wgrad(D, X, n):
    """per-sample s[S, co, ci, ky, kx] = sum_yx D[S, co, y, x] Xpad[S, ci, y + ky, x + kx], 'same' padding of an n x n tap"""
    pad = n // 2
    H, W_ = D.shape[2:]
    Xp = np.pad(X, ((0, 0), (0, 0), (pad, pad), (pad, pad)))
    out = np.zeros((D.shape[0], D.shape[1], X.shape[1], n, n))
    for ky in range(n):
        for kx in range(n):
            out[:, :, :, ky, kx] = np.einsum('scyx,sdyx->scd', D, Xp[:, :, ky:ky + H, kx:kx + W_])
    return out


def _dgrad(D, Wt):
    """dX[S, ci, y, x] = sum_(co, ky, kx) D[S, co, y - ky + 1, x - kx + 1] W[co, ci, ky, kx] (3 x 3, 'same')"""
    H, W_ = D.shape[2:]
    Dp = np.pad(D, ((0, 0), (0, 0), (1, 1), (1, 1)))
    out = np.zeros((D.shape[0], Wt.shape[1], H, W_))
    for ky in range(3):
        for kx in range(3):
            out += np.einsum('scyx,cd->sdyx', Dp[:, :, 2 - ky:2 - ky + H, 2 - kx:2 - kx + W_], Wt[:, :, ky, kx])
    return out


def _bilinear(op, a, ea, b, eb, K):
    """(op(a, b), the chain bound of the docstring) for a bilinear ``op`` whose sums have at most K terms"""
    aa, ab = np.abs(a), np.abs(b)
    return op(a, b), gamma(K + 1) * op(aa + ea, ab + eb) + op(aa, eb) + op(ea, ab) + op(ea, eb)


def _sum_b(t, e):
    """the sum chain over the samples and its bound"""
    return t.sum(axis=0), gamma(len(t)) * (np.abs(t) + e).sum(axis=0) + e.sum(axis=0)


def backward64(params, acts64, dlogits):
    """(grads, bounds): name -> float64 gradient and name -> the derived bound on |float32 chain - that|, same shapes"""
    q = {k: v.astype(np.float64) for k, v in params.items()}
    g = np.asarray(dlogits, F).astype(np.float64).reshape(-1)
    (a, ea), (u, eu), (c1, e1), (c2, e2), (cat, ecat), (f2, ef2) = (acts64[k] for k in ('a', 'u', 'c1', 'c2', 'cat', 'f2'))
    i1, i2 = acts64['i1'], acts64['i2']
    S, C1, H1, W1 = c1.shape
    C2, H2, W2 = c2.shape[1:]
    F1, F2 = q['fc1.weight'].shape[0], q['fc2.weight'].shape[0]
    m = S
    zero = np.zeros
    ow = q['out.weight'][0]
    # dz2 = g ow: one product, K = 1
    t = g[:, None] * ow[None, :]
    dz2, edz2 = np.where(f2 > 0, t, 0.0), np.where(f2 > 0, gamma(2) * np.abs(t), 0.0)
    t, e = _bilinear(lambda x, w_: x @ w_, dz2, edz2, q['fc2.weight'], zero(q['fc2.weight'].shape), F2)
    dzc, edzc = np.where(cat > 0, t, 0.0), np.where(cat > 0, e, 0.0)
    c2f, e2f = c2.reshape(S, -1), e2.reshape(S, -1)
    t, e = _bilinear(lambda x, w_: x @ w_, dzc[:, :F1], edzc[:, :F1], q['fc1.weight'], zero(q['fc1.weight'].shape), F1)
    ok2 = c2 > 0
    g2, eg2 = np.where(ok2, t.reshape(c2.shape), 0.0), np.where(ok2, e.reshape(c2.shape), 0.0)
    D2, eD2 = _unpool(g2, i2, ok2), _unpool(eg2, i2, ok2)
    s2, es2 = _bilinear(lambda d, x: _wgrad(d, x, 3), D2, eD2, c1, e1, H2 * W2)
    s2b, es2b = D2.sum(axis=(2, 3)), gamma(H2 * W2) * (np.abs(D2) + eD2).sum(axis=(2, 3)) + eD2.sum(axis=(2, 3))
    t, e = _bilinear(_dgrad, D2, eD2, q['conv2.weight'], zero(q['conv2.weight'].shape), 9 * C2)
    ok1 = c1 > 0
    g1, eg1 = np.where(ok1, t, 0.0), np.where(ok1, e, 0.0)
    D1, eD1 = _unpool(g1, i1, ok1), _unpool(eg1, i1, ok1)
    s1, es1 = _bilinear(lambda d, x: _wgrad(d, x, 5), D1, eD1, a[:, None], ea[:, None], H1 * W1)
    s1b, es1b = D1.sum(axis=(2, 3)), gamma(H1 * W1) * (np.abs(D1) + eD1).sum(axis=(2, 3)) + eD1.sum(axis=(2, 3))

    def fc(dy, edy, x, ex):
        return _bilinear(lambda p_, r: p_.T @ r, dy, edy, x, ex, m)
    G, B = {}, {}
    G['out.weight'], B['out.weight'] = fc(g[:, None], zero((S, 1)), f2, ef2)
    G['out.bias'], B['out.bias'] = _sum_b(g[:, None], zero((S, 1)))
    G['fc2.weight'], B['fc2.weight'] = fc(dz2, edz2, cat, ecat)
    G['fc2.bias'], B['fc2.bias'] = _sum_b(dz2, edz2)
    G['pose.weight'], B['pose.weight'] = fc(dzc[:, F1:], edzc[:, F1:], u[:, None], eu[:, None])
    G['pose.bias'], B['pose.bias'] = _sum_b(dzc[:, F1:], edzc[:, F1:])
    G['fc1.weight'], B['fc1.weight'] = fc(dzc[:, :F1], edzc[:, :F1], c2f, e2f)
    G['fc1.bias'], B['fc1.bias'] = _sum_b(dzc[:, :F1], edzc[:, :F1])
    G['conv2.weight'], B['conv2.weight'] = _sum_b(s2, es2)
    G['conv2.bias'], B['conv2.bias'] = _sum_b(s2b, es2b)
    G['conv1.weight'], B['conv1.weight'] = _sum_b(s1, es1)
    G['conv1.bias'], B['conv1.bias'] = _sum_b(s1b, es1b)
    return G, B


def take(acts, keep):
    """the samples ``keep`` (bool or index array) of an ``acts`` dict of either precision"""
    out = {}
    for k, v in acts.items():
        out[k] = (v[0][keep], v[1][keep]) if isinstance(v, tuple) else v[keep]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# Adam

def adam_constants(step, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
    """(lr, beta1, beta2, eps, corr1, corr2) as float32, the corrections from the float32 betas in float64 (lib.adam_params)"""
    b1, b2 = float(F(betas[0])), float(F(betas[1]))
    return F(lr), F(b1), F(b2), F(eps), F(1.0 / (1.0 - b1 ** step)), F(1.0 / (1.0 - b2 ** step))


def adam(w, g, m, v, consts):
    """k_adam_step: (w', m', v') float32"""
    lr, b1, b2, eps, c1, c2 = consts
    w, g, m, v = (np.ascontiguousarray(t, F) for t in (w, g, m, v))
    omb1, omb2 = F(F(1) - b1), F(F(1) - b2)
    m1 = fma(np.full_like(m, b1), m, (omb1 * g).astype(F))
    v1 = fma(np.full_like(v, b2), v, ((omb2 * g).astype(F) * g).astype(F))
    num = (lr * (m1 * c1).astype(F)).astype(F)
    den = (np.sqrt((v1 * c2).astype(F)).astype(F) + eps).astype(F)
    return (w - (num / den).astype(F)).astype(F), m1, v1


def adam64(w, g, m, v, consts):
    """(w', bound) in float64 from the float32 inputs and constants: the update and the docstring's ew"""
    lr, b1, b2, eps, c1, c2 = (float(t) for t in consts)
    w, g, m, v = (np.asarray(t, F).astype(np.float64) for t in (w, g, m, v))
    m1 = b1 * m + (1.0 - b1) * g
    v1 = b2 * v + (1.0 - b2) * g * g
    em = gamma(3) * (np.abs(b1 * m) + np.abs((1.0 - b1) * g))
    ev = gamma(4) * (b2 * v + (1.0 - b2) * g * g)
    mh, vh = m1 * c1, v1 * c2
    emh = c1 * em * (1 + U) + U * np.abs(mh)
    evh = c2 * ev * (1 + U) + U * vh
    s = np.sqrt(vh)
    with np.errstate(invalid='ignore', divide='ignore'):
        es = np.where(vh > 0, evh / s, 0.0)
    es = es + U * (s + es)
    d = s + eps
    ed = es + U * (d + es)
    n = lr * mh
    en = lr * emh * (1 + U) + U * np.abs(n)
    qv = n / d
    eq = ((en + np.abs(qv) * ed) / (d - ed)) * (1 + U) + U * np.abs(qv)
    w1 = w - qv
    return w1, eq + U * (np.abs(w1) + eq)
