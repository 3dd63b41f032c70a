"""NumPy restatement of csrc/rv_dev_grasp_quality.h (rv_grasp_quality), for the tests: float32, operation for operation.
Every dot product is one FMA chain that starts from the bias and takes its terms in ascending input index (channel, tap
row, tap column for the convolutions), with the exact ``fma`` of tests/cem_host.py; it is vectorised over samples and
outputs and sequential over k.  relu(v) = v > 0 ? v : 0, pool2 = the maximum of the 2 x 2 window after relu.

``forward64`` evaluates the same network in float64 and returns, beside every logit, a DERIVED bound B on the error of any
float32 evaluation of it.  Derivation, with u = 2^-24 and gamma_n = n u / (1 - n u) (Higham, Accuracy and Stability of
Numerical Algorithms, §3.1: a sum of K products accumulated in any order, fused or not, from a bias, has error at most
gamma_(K+1) (|W| |x| + |b|) in the values it was given):
  * normalisation a = fl(fl(x - m) s): two roundings, |a^ - a| <= gamma_2 |a|;
  * a layer y = W x + b whose float32 input x^ has |x^ - x| <= e:  |y^ - y| <= gamma_(K+1) (|W| (|x| + e) + |b|) + |W| e
    (the first term is the rounding of the chain on the input it saw, |x^| <= |x| + e; the second is what the input's own
    error does to the exact sum);
  * relu and the 2 x 2 maximum are 1-Lipschitz: relu keeps e, the maximum takes the largest e of its window.
The bound of the logit is B.  float64's own rounding (2^-29 of float32's) is inside the slack between gamma_K, which
the K-term chain needs, and gamma_(K+1), which is used.  A float32 evaluation in another order (torch) obeys the same
bound, so two float32 evaluations differ by at most 2 B."""
import numpy as np

from cem_host import fma

F = np.float32
U = 2.0 ** -24


def gamma(n):
    return n * U / (1.0 - n * U)


def relu(v):
    return np.where(v > 0, v, F(0)).astype(v.dtype)


def pool2(r):
    """2 x 2 maximum over the last two axes, in the kernel's order: m = v00; v01 > m; v10 > m; v11 > m"""
    m = r[..., 0::2, 0::2]
    for b in (r[..., 0::2, 1::2], r[..., 1::2, 0::2], r[..., 1::2, 1::2]):
        m = np.where(b > m, b, m)
    return m


def _chain(acc, terms):
    """acc = fma(x_k, w_k, acc) over ``terms`` (an iterable of (x_k, w_k) that broadcast against acc), in order"""
    for x, w in terms:
        acc = fma(x, w, acc)
    return acc


def forward(params, norm, images, depths, chunk=16):
    """logits float32 [S] of ``images`` [S, h, w] and ``depths`` [S]; ``params``: GraspQualityModel.params (torch's natural
    layouts); ``norm``: its four float32 constants.  Samples are independent: they are evaluated ``chunk`` at a time."""
    images = np.ascontiguousarray(images, F)
    depths = np.ascontiguousarray(depths, F).reshape(-1)
    out = [_forward(params, norm, images[i:i + chunk], depths[i:i + chunk]) for i in range(0, len(images), chunk)]
    return np.concatenate(out).astype(F)


def _forward(q, norm, x, z):
    S, h, w = x.shape
    with np.errstate(invalid='ignore', over='ignore'):
        a = ((x - F(norm['im_mean'])).astype(F) * F(norm['im_inv_std'])).astype(F)
        u = ((z - F(norm['z_mean'])).astype(F) * F(norm['z_inv_std'])).astype(F)
        # conv1 5 x 5, zero padding of the normalised image
        w1, b1 = q['conv1.weight'], q['conv1.bias']
        C1 = w1.shape[0]
        ap = np.zeros((S, h + 4, w + 4), F)
        ap[:, 2:-2, 2:-2] = a
        acc = np.broadcast_to(b1[None, :, None, None], (S, C1, h, w)).astype(F)
        acc = _chain(acc, ((ap[:, None, ky:ky + h, kx:kx + w], w1[None, :, 0, ky, kx, None, None])
                           for ky in range(5) for kx in range(5)))
        c1 = pool2(relu(acc))
        # conv2 3 x 3 over (channel, tap row, tap column)
        w2, b2 = q['conv2.weight'], q['conv2.bias']
        C2 = w2.shape[0]
        H1, W1 = h // 2, w // 2
        cp = np.zeros((S, C1, H1 + 2, W1 + 2), F)
        cp[:, :, 1:-1, 1:-1] = c1
        acc = np.broadcast_to(b2[None, :, None, None], (S, C2, H1, W1)).astype(F)
        acc = _chain(acc, ((cp[:, ci, None, ky:ky + H1, kx:kx + W1], w2[None, :, ci, ky, kx, None, None])
                           for ci in range(C1) for ky in range(3) for kx in range(3)))
        c2 = pool2(relu(acc))
        flat = c2.reshape(S, -1)          # channel-major
        f1 = relu(_fc(flat, q['fc1.weight'], q['fc1.bias']))
        p = relu(_fc(u[:, None], q['pose.weight'], q['pose.bias']))
        f2 = relu(_fc(np.concatenate([f1, p], axis=1), q['fc2.weight'], q['fc2.bias']))
        return _fc(f2, q['out.weight'], q['out.bias'])[:, 0]


def _fc(x, w, b):
    acc = np.broadcast_to(b[None, :], (x.shape[0], w.shape[0])).astype(F)
    return _chain(acc, ((x[:, k, None], w[None, :, k]) for k in range(w.shape[1])))


# ---------------------------------------------------------------------------------------------------------------------
# float64 evaluation with the running error bound

def _layer64(x, e, w, b, K, conv=None):
    """(y, e_y) of y = W x + b in float64; x, e [S, ...]; conv: None for fc, else the padding of a 'same' convolution"""
    g = gamma(K + 1)
    w = w.astype(np.float64); b = b.astype(np.float64)
    if conv is None:
        y = x @ w.T + b
        mag = (np.abs(x) + e) @ np.abs(w).T + np.abs(b)
        prop = e @ np.abs(w).T
        return y, g * mag + prop
    pad = conv
    S, Ci, H, W_ = x.shape
    Co = w.shape[0]
    xp = np.pad(x, ((0, 0), (0, 0), (pad, pad), (pad, pad)))
    ep = np.pad(e, ((0, 0), (0, 0), (pad, pad), (pad, pad)))
    y = np.broadcast_to(b[None, :, None, None], (S, Co, H, W_)).copy()
    mag = np.broadcast_to(np.abs(b)[None, :, None, None], (S, Co, H, W_)).copy()
    prop = np.zeros((S, Co, H, W_))
    n = 2 * pad + 1
    for ci in range(Ci):
        for ky in range(n):
            for kx in range(n):
                xs, es = xp[:, ci, None, ky:ky + H, kx:kx + W_], ep[:, ci, None, ky:ky + H, kx:kx + W_]
                wk = w[None, :, ci, ky, kx, None, None]
                y += xs * wk
                mag += (np.abs(xs) + es) * np.abs(wk)
                prop += es * np.abs(wk)
    return y, g * mag + prop


def _pool64(y, e):
    def win(t):
        return np.stack([t[..., 0::2, 0::2], t[..., 0::2, 1::2], t[..., 1::2, 0::2], t[..., 1::2, 1::2]]).max(axis=0)
    return win(y), win(e)


def forward64(params, norm, images, depths):
    """(logits float64 [S], B float64 [S]): the network in float64 on the float32 inputs, and the bound of the docstring"""
    q = params
    x = np.asarray(images, F).astype(np.float64)
    z = np.asarray(depths, F).astype(np.float64).reshape(-1)
    a = (x - float(norm['im_mean'])) * float(norm['im_inv_std'])
    u = (z - float(norm['z_mean'])) * float(norm['z_inv_std'])
    ea, eu = gamma(2) * np.abs(a), gamma(2) * np.abs(u)
    y, e = _layer64(a[:, None], ea[:, None], q['conv1.weight'], q['conv1.bias'], 25, conv=2)
    c1, e1 = _pool64(np.maximum(y, 0), e)
    y, e = _layer64(c1, e1, q['conv2.weight'], q['conv2.bias'], 9 * c1.shape[1], conv=1)
    c2, e2 = _pool64(np.maximum(y, 0), e)
    S = len(x)
    y, e = _layer64(c2.reshape(S, -1), e2.reshape(S, -1), q['fc1.weight'], q['fc1.bias'], q['fc1.weight'].shape[1])
    f1, ef1 = np.maximum(y, 0), e
    y, e = _layer64(u[:, None], eu[:, None], q['pose.weight'], q['pose.bias'], 1)
    p, ep = np.maximum(y, 0), e
    cat, ecat = np.concatenate([f1, p], axis=1), np.concatenate([ef1, ep], axis=1)
    y, e = _layer64(cat, ecat, q['fc2.weight'], q['fc2.bias'], cat.shape[1])
    f2, ef2 = np.maximum(y, 0), e
    y, e = _layer64(f2, ef2, q['out.weight'], q['out.bias'], f2.shape[1])
    return y[:, 0], e[:, 0]


# ---------------------------------------------------------------------------------------------------------------------
# seeded inputs

def sample_inputs(seed, count, h, w):
    """(images [count, h, w], depths [count]) float32: depth-like values around 0.6 m with a bump, a quarter of the pixels
    exactly 0 (what rv_grasp_crops writes outside the image), grasp depths around 0.55 m"""
    rng = np.random.RandomState(seed)
    img = (0.6 + 0.05 * rng.standard_normal((count, h, w))).astype(F)
    img[rng.uniform(size=img.shape) < 0.25] = 0
    return img, (0.55 + 0.05 * rng.standard_normal(count)).astype(F)
