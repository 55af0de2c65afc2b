"""Float64 numpy witness of the fused MLP (csrc/ffmlp.hip, csrc/ffmlp_generic.hip) and of the elementwise NGP head kernels
(csrc/ngp_head.hip), written from the mathematics and from the rounding points those files document.

Network: flat weights `[W, in] | (n - 1) x [W, W] | [16, W]`, row-major, no biases.  Per layer the kernels compute
`a = h(f(h(x M^T)))` — h = rounding to binary16, ties to even; the sum in fp32 — and for the backward pass, from the stored
post-activation value a, `d = h(f'(a) h(g M))`; `grad_inputs = h(d_1 M_0)`, `grad_weights = h(sum_b d[b]^T x[b])`.  The backward
pass ignores the output activation (the interface's contract: the caller hands in the gradient of the pre-activation output).

Exact cases: when every value at a layer boundary is an integer of magnitude <= 2,048 (exactly representable in binary16) and the
absolute products of every sum add up to less than 2^24 (every fp32 partial sum exact, in any order), the kernels have to equal this
witness BIT FOR BIT whatever their accumulation order, tile walk or grid.  `assert_exact` checks those conditions on a case's own
data, so that a test never relies on them by faith.

Everything here is numpy float64; no torch arithmetic."""
import numpy as np

K_ACT = 10.0  # the scale of squareplus / softplus
RELU, EXP, SINE, SIGMOID, SQUAREPLUS, SOFTPLUS, NONE = range(7)
ACT_NAMES = ("relu", "exp", "sine", "sigmoid", "squareplus", "softplus", "none")


def h16(v):
    """round to binary16 (ties to even), back in float64"""
    with np.errstate(over="ignore"):
        return np.asarray(v, np.float64).astype(np.float16).astype(np.float64)


def ulp16(v):
    """spacing of binary16 at |v| (2^-24 in the subnormal range)"""
    a = np.abs(np.asarray(v, np.float64))
    _, e = np.frexp(np.maximum(a, 2.0 ** -14))  # |v| = m 2^e, m in [0.5, 1)
    return np.ldexp(1.0, e - 11)


def act_fwd(a, x):
    if a == RELU:
        return np.where(x > 0, x, 0.0)
    if a == EXP:
        return np.exp(x)
    if a == SINE:
        return np.sin(x)
    if a == SIGMOID:
        return 1.0 / (1.0 + np.exp(-x))
    if a == SQUAREPLUS:  # (x + sqrt(x^2 + 4 / k^2)) / 2
        return 0.5 * (x + np.sqrt(x * x + 4.0 / (K_ACT * K_ACT)))
    if a == SOFTPLUS:    # log(1 + e^(k x)) / k
        return np.logaddexp(0.0, K_ACT * x) / K_ACT
    if a == NONE:
        return x
    raise ValueError(f"activation {a}")


def act_bwd(a, g, y):
    """g f'(x) written through the stored value y = f(x):
    exp: f' = y.  sigmoid: f' = y (1 - y).  softplus: f' = e^(kx) / (1 + e^(kx)) = 1 - e^(-k y).
    squareplus: u = k y solves u^2 - (k x) u - 1 = 0, so k x = u - 1/u, sqrt((k x)^2 + 4) = u + 1/u and
    f' = (1 + k x / sqrt((k x)^2 + 4)) / 2 = u^2 / (u^2 + 1).  sine: not a function of y — no backward."""
    if a == RELU:
        return np.where(y > 0, g, 0.0)
    if a == EXP:
        return g * y
    if a == SIGMOID:
        return g * (y * (1.0 - y))
    if a == SQUAREPLUS:
        u2 = (K_ACT * y) ** 2
        return g * (u2 / (u2 + 1.0))
    if a == SOFTPLUS:
        return g * -np.expm1(-K_ACT * y)
    if a == NONE:
        return g
    raise ValueError(f"activation {a} has no backward from the stored value")


def split(w, in_dim, W, n):
    """the matrices of a flat weight vector: [W, in], (n - 1) x [W, W], [16, W]"""
    mats, off = [], 0
    for o, k in [(W, in_dim)] + [(W, W)] * (n - 1) + [(16, W)]:
        mats.append(w[off:off + o * k].reshape(o, k))
        off += o * k
    assert off == len(w)
    return mats


def flat(mats):
    return np.concatenate([np.asarray(m, np.float64).reshape(-1) for m in mats])


def forward(x, mats, act, out_act=NONE, rounding=True, shift=None):
    """-> dict(pre, acts, out_pre, out).  `shift[l]`: stored activation l moved by that many binary16 ulps (sensitivity probes)."""
    r = h16 if rounding else (lambda v: v)
    cur, pre, acts = np.asarray(x, np.float64), [], []
    for l, m in enumerate(mats[:-1]):
        p = r(cur @ m.T)
        a = r(act_fwd(act, p))
        if shift is not None and shift[l]:
            a = a + shift[l] * ulp16(a)
        pre.append(p)
        acts.append(a)
        cur = a
    out_pre = r(cur @ mats[-1].T)
    return dict(pre=pre, acts=acts, out_pre=out_pre, out=r(act_fwd(out_act, out_pre)))


def backward(grad, x, mats, acts, act, rounding=True):
    """-> dict(g, d, grad_inputs, gw): g[l] / d[l] the gradient w.r.t. hidden layer l's post- / pre-activation, gw[m] the UNROUNDED
    float64 weight gradient of matrix m (the caller rounds: an accumulating call rounds pre-fill + sum once)"""
    r = h16 if rounding else (lambda v: v)
    n = len(mats) - 1
    g, d = [None] * n, [None] * n
    up = np.asarray(grad, np.float64)
    gw = [None] * (n + 1)
    gw[n] = up.T @ acts[n - 1]
    for l in range(n - 1, -1, -1):
        g[l] = r(up @ mats[l + 1])
        d[l] = r(act_bwd(act, g[l], acts[l]))
        gw[l] = d[l].T @ (acts[l - 1] if l else np.asarray(x, np.float64))
        up = d[l]
    return dict(g=g, d=d, grad_inputs=r(d[0] @ mats[0]), gw=gw)


# ---------------------------------------------------------------------------------------------------------------- exact cases
def _sparse_matrix(rng, rows, cols, nnz=2, positive=0.5):
    """entries in {0, +-1}, at most `nnz` non-zeros per row; the columns of each pass come from random permutations, so every
    column is used equally often"""
    m = np.zeros((rows, cols))
    for _ in range(nnz):
        c = np.concatenate([rng.permutation(cols) for _ in range(-(-rows // cols))])[:rows]
        m[np.arange(rows), c] = np.where(rng.random(rows) < positive, 1.0, -1.0)
    return m


def _dense_matrix(rng, rows, cols):
    return rng.integers(-1, 2, (rows, cols)).astype(np.float64)


def make_case(kind, in_dim, W, n, B, act, out=16, seed=0):
    """kind "sparse": every matrix sparse; "dense": first and last matrix dense in {-1, 0, 1}, hidden ones sparse.
    Inputs and output gradients in {-1, 0, 1}; rows >= out of the last matrix and columns >= out of the gradient are zero."""
    rng = np.random.default_rng([seed, in_dim, W, n, act, kind == "dense"])
    # under ReLU a hidden layer's inputs are non-negative: more positive weights keep 20 - 80 % of the gates open at any depth
    pos = 0.62 if act == RELU else 0.5
    if kind == "dense":
        mats = [_dense_matrix(rng, W, in_dim)] + [_sparse_matrix(rng, W, W, 2, pos) for _ in range(n - 1)] + [_dense_matrix(rng, 16, W)]
    else:
        # (first / last matrix: enough entries per row that a wide input or hidden layer still gets a gradient everywhere)
        mats = ([_sparse_matrix(rng, W, in_dim, max(2, in_dim // 16))] + [_sparse_matrix(rng, W, W, 2, pos) for _ in range(n - 1)]
                + [_sparse_matrix(rng, 16, W, max(2, W // 8))])
    mats[-1][out:] = 0
    x = rng.integers(-1, 2, (B, in_dim)).astype(np.float64)
    grad = rng.integers(-1, 2, (B, 16)).astype(np.float64)
    grad[:, out:] = 0
    return dict(kind=kind, in_dim=in_dim, W=W, n=n, B=B, act=act, out=out, mats=mats, x=x, grad=grad)


def run_case(case, rows=None, out_act=NONE):
    """the witness's results on the first `rows` rows (all by default): outputs, grad_inputs (rounded), gw (flat float64 sums)"""
    x, grad = case["x"][:rows], case["grad"][:rows]
    f = forward(x, case["mats"], case["act"], out_act)
    b = backward(grad, x, case["mats"], f["acts"], case["act"])
    return dict(f=f, b=b, outputs=f["out"], grad_inputs=b["grad_inputs"], gw=flat(b["gw"]))


def assert_exact(case, rows=None):
    """the conditions under which the kernels must equal the witness bit for bit, on the case's own data; returns run_case()"""
    mats, act, out, n = case["mats"], case["act"], case["out"], case["n"]
    x, grad = case["x"][:rows], case["grad"][:rows]
    tag = f"{case['kind']} {case['in_dim']}x{case['W']}x{n} act {act} B {len(x)}"
    res = run_case(case, rows)
    f, b = res["f"], res["b"]
    exact = forward(x, mats, act, rounding=False)
    eb = backward(grad, x, mats, exact["acts"], act, rounding=False)

    def small_int(name, v, ref):
        assert np.array_equal(v, ref), f"{tag}: {name} changes under rounding"
        assert np.array_equal(v, np.rint(v)) and np.abs(v).max() <= 2048, f"{tag}: {name} not an integer <= 2048 ({np.abs(v).max()})"

    def sum_ok(name, a, m):
        s = (np.abs(a) @ np.abs(m)).max()
        assert s < 2.0 ** 24, f"{tag}: {name} sums {s} of absolute products"

    cur = x
    for l in range(n):
        small_int(f"pre-activation {l}", f["pre"][l], exact["pre"][l])
        small_int(f"activation {l}", f["acts"][l], exact["acts"][l])
        small_int(f"gradient g {l}", b["g"][l], eb["g"][l])
        small_int(f"gradient d {l}", b["d"][l], eb["d"][l])
        sum_ok(f"layer {l}", cur, mats[l].T)
        sum_ok(f"data gradient {l}", b["d"][l + 1] if l + 1 < n else grad, mats[l + 1])
        sum_ok(f"weight gradient {l}", b["d"][l].T, cur)
        cur = f["acts"][l]
    small_int("outputs", f["out"], exact["out"])
    small_int("grad_inputs", b["grad_inputs"], eb["grad_inputs"])
    sum_ok("output layer", cur, mats[n].T)
    sum_ok("grad_inputs", b["d"][0], mats[0])
    sum_ok("weight gradient of the output layer", grad.T, cur)
    for m in range(n + 1):
        assert np.array_equal(b["gw"][m], np.rint(b["gw"][m])) and np.abs(b["gw"][m]).max() <= 65504, f"{tag}: weight gradient {m} overflows binary16"

    def live(name, v, lo=0.2):
        frac = float((v != 0).mean())
        assert frac >= lo, f"{tag}: only {100 * frac:.1f} % of {name} non-zero"

    live("outputs", f["out"][:, :out])
    live("grad_inputs", b["grad_inputs"])
    live("grad_weights", np.concatenate([g.reshape(-1) for g in b["gw"][:n]] + [b["gw"][n][:out].reshape(-1)]))
    for m in range(n + 1):
        live(f"weight gradient {m}", b["gw"][m][:out] if m == n else b["gw"][m], 0.1)
    if act == RELU:
        for l in range(n):
            open_ = float((f["acts"][l] > 0).mean())
            assert 0.2 <= open_ <= 0.8, f"{tag}: {100 * open_:.1f} % of hidden layer {l}'s gates open"
    return res


# The shapes (in_dim, W, n_layers) of the exact-parity tests, chosen from the launch code so that every instantiation family is
# entered at its smallest shape (tests/test_gpu_ffmlp_exact.py)
NATIVE_SHAPES = [(16, 32, 2), (48, 32, 3), (64, 32, 2), (32, 32, 4), (16, 64, 2), (32, 64, 2), (32, 64, 3), (48, 64, 2), (64, 64, 4),
                 (32, 64, 7), (32, 128, 2), (64, 128, 4), (128, 128, 2), (144, 128, 2), (160, 128, 3)]
# ... of which the re-computing fused backward takes: widths 32 / 64, at most 3 / 2 hidden matrices
FUSED_SHAPES = [(16, 32, 2), (48, 32, 3), (64, 32, 2), (32, 32, 4), (16, 64, 2), (32, 64, 2), (32, 64, 3), (48, 64, 2)]
# layer-by-layer path; (32, 128, 6): 8 + 5 x 32 + 8 = 176 KiB of forward weight fragments, beyond the 144 KiB budget of ffmlp_native_shape
GENERIC_SHAPES = [(32, 16, 2), (16, 16, 3), (64, 256, 2), (128, 64, 2), (80, 32, 3), (176, 128, 2), (32, 128, 6)]
BIG_SHAPES = [(32, 64, 2), (32, 64, 3), (160, 128, 3)]  # also at 131,200 rows: above every grid cap of the launch code
BATCHES, BIG_BATCH = (128, 384, 4736), 131200
REAL_OUT = {(32, 64, 3): 3, (64, 64, 4): 8, (64, 128, 4): 5, (160, 128, 3): 3, (64, 256, 2): 3, (48, 32, 3): 7}  # else 16
SEEDS = {("sparse", (32, 16, 2), 0): 3}  # (kind, shape, act) -> seed, where seed 0 does not meet assert_exact's conditions


def exact_case(kind, shape, act, B):
    """the case of a shape with B rows; the tests take the smaller batches as the leading rows of the 4,736-row case
    (`rows` of run_case / assert_exact), so one case serves 128, 384 and 4,736 rows and the n_valid runs"""
    return make_case(kind, *shape, B, act, REAL_OUT.get(shape, 16), SEEDS.get((kind, shape, act), 0))


# ------------------------------------------------------------------------------------------------- rounding / accumulation probes
def probe_case(act, B=128, seed=0):
    """(32, 64, 2) network whose first hidden layer and output layer each hold the exact sums 2,049 / 2,050 / 2,051 (stored as
    2,048 / 2,050 / 2,052: ties to even) and a row 2,048 + 16 x 1 - 2,048 (16 in fp32 in any order; a binary16 accumulator loses
    the ones).  Every batch row is that pattern times +-1, so under ReLU half the rows are closed.
    -> (case, expected first-layer values of units 0..3 for a + row, expected outputs 0..7 for a + row)"""
    rng = np.random.default_rng(seed)
    in_dim, W, n = 32, 64, 2
    base = np.zeros(in_dim)
    base[0], base[1], base[2], base[3], base[31] = 2048, 1, 2, 3, 2048  # (the -2,048 comes last in index order)
    base[5:21] = 1
    m0 = np.zeros((W, in_dim))
    m0[0, [0, 1]] = 1            # 2049 -> 2048
    m0[1, [0, 2]] = 1            # 2050
    m0[2, [0, 3]] = 1            # 2051 -> 2052
    m0[3, 0], m0[3, 5:21], m0[3, 31] = 1, 1, -1  # 2048 + 16 - 2048 = 16
    m0[4, 0], m0[5, 1], m0[6, 2], m0[7, 3] = 1, 1, 1, 1  # 2048, 1, 2, 3
    for r in range(8, W):
        m0[r, rng.integers(5, in_dim - 1)] = rng.choice([-1.0, 1.0])
    perm = np.concatenate([rng.permutation(8), 8 + rng.permutation(W - 8)])  # hidden unit u -> second-layer unit perm[u]
    m1 = np.zeros((W, W))
    m1[perm, np.arange(W)] = np.concatenate([np.ones(8), rng.choice([-1.0, 1.0], W - 8)])
    m2 = np.zeros((16, W))
    for o in range(4):
        m2[o, perm[o]] = 1                       # the first layer's probes, unchanged
    for o, u in ((4, 5), (5, 6), (6, 7)):        # 2048 + 1 / 2 / 3 in the output layer
        m2[o, perm[4]], m2[o, perm[u]] = 1, 1
    m2[7, perm[4]], m2[7, perm[8:24]], m2[7, perm[0]] = 1, 1, -1  # 2048 + sixteen (+-1 or 0) - 2048
    sign = rng.choice([-1.0, 1.0], B)
    sign[:2] = (1.0, -1.0)
    x = sign[:, None] * base[None, :]
    case = dict(kind="probe", in_dim=in_dim, W=W, n=n, B=B, act=act, out=16, mats=[m0, m1, m2], x=x, grad=np.zeros((B, 16)), sign=sign)
    return case, np.array([2048.0, 2050.0, 2052.0, 16.0]), np.array([2048.0, 2050.0, 2052.0, 16.0, 2048.0, 2050.0, 2052.0])


# ---------------------------------------------------------------------------------------------------------- activation chains
def chain_case(in_dim, W, act, B=128, seed=0):
    """two hidden layers; every output is an elementwise expression of one first-layer pre-activation p1 (an integer in [-3, 3]):
    first matrix sparse integer (<= 3 entries +-1 per row), second a signed permutation scaled 2^-s1, third a signed selection
    scaled 2^-s2 — every product after the first layer is exact, so only the activations' own rounding is left.
    s1 = 3 under exp (a1 <= e^3, a2 <= e^2.6; weight-gradient sums stay far below 65,504), 1 otherwise; s2 = 1."""
    rng = np.random.default_rng([seed, in_dim, W, act])
    s1, s2 = (3, 1) if act == EXP else (1, 1)
    m0 = _sparse_matrix(rng, W, in_dim, 3)
    m1 = np.zeros((W, W))
    m1[rng.permutation(W), np.arange(W)] = rng.choice([-1.0, 1.0], W) * 2.0 ** -s1
    m2 = np.zeros((16, W))
    m2[np.arange(16), rng.permutation(W)[:16]] = rng.choice([-1.0, 1.0], 16) * 2.0 ** -s2
    x = rng.integers(-1, 2, (B, in_dim)).astype(np.float64)
    grad = rng.integers(-1, 2, (B, 16)).astype(np.float64)
    return dict(kind="chain", in_dim=in_dim, W=W, n=2, B=B, act=act, out=16, mats=[m0, m1, m2], x=x, grad=grad)


SHIFTS = [(a, b) for a in (-1, 0, 1) for b in (-1, 0, 1)]


def chain_bounds(case, out_act=NONE):
    """reference values and per-element bounds of a chain case, from the witness alone.

    The kernels evaluate f in fp32 (error ~2^-22 relative), the witness in float64, so a stored activation differs from the
    witness's by a rounding flip of one binary16 ulp at most.  Every compared quantity is re-evaluated with the two stored
    activations moved by -1 / 0 / +1 ulp (nine combinations); per element,
        bound = 2 (largest deviation among the combinations + one binary16 ulp of the reference value)
    — the factor 2 for the second-order term and the fp32 evaluation error of expf / logf / sqrtf.
    Sums (grad_inputs over the <= W terms of a column of the first matrix, grad_weights over the batch) take that bound PER TERM,
    summed, plus terms x 2^-24 x sum|term| for the order of the fp32 additions, plus one ulp of the reference sum (its own
    rounding)."""
    mats, act, x, grad = case["mats"], case["act"], case["x"], case["grad"]
    B = len(x)
    assert np.abs(forward(x, mats, NONE)["pre"][0]).max() <= 3

    def evaluate(shift):
        f = forward(x, mats, act, out_act, shift=shift)
        r = dict(out=f["out"])
        if act != SINE:
            b = backward(grad, x, mats, f["acts"], act)
            ins = [x, f["acts"][0], f["acts"][1]]
            ups = [b["d"][0], b["d"][1], grad]
            r.update(d0=b["d"][0], terms=[ups[m][:, :, None] * ins[m][:, None, :] for m in range(3)], grad_inputs=b["grad_inputs"], gw=b["gw"])
        return r

    ref = evaluate(None)
    dev = {k: np.zeros_like(ref[k]) for k in ("out", "d0") if k in ref}
    tdev = [np.zeros_like(t) for t in ref.get("terms", [])]
    for s in SHIFTS:
        if s == (0, 0):
            continue
        r = evaluate(s)
        for k in dev:
            dev[k] = np.maximum(dev[k], np.abs(r[k] - ref[k]))
        for m in range(len(tdev)):
            tdev[m] = np.maximum(tdev[m], np.abs(r["terms"][m] - ref["terms"][m]))
    res = dict(out=ref["out"], out_bound=2 * (dev["out"] + ulp16(ref["out"])))
    if act != SINE:
        d0_bound = 2 * (dev["d0"] + ulp16(ref["d0"]))  # per term of grad_inputs: the stored first-layer gradient
        nterms = int((mats[0] != 0).sum(0).max())
        res["grad_inputs"] = ref["grad_inputs"]
        res["grad_inputs_bound"] = (d0_bound @ np.abs(mats[0]) + nterms * 2.0 ** -24 * (np.abs(ref["d0"]) @ np.abs(mats[0]))
                                    + ulp16(ref["grad_inputs"]))
        gws, bounds = [], []
        for m in range(3):
            t = ref["terms"][m]
            gws.append(h16(ref["gw"][m]))
            bounds.append((2 * (tdev[m] + ulp16(t))).sum(0) + B * 2.0 ** -24 * np.abs(t).sum(0) + ulp16(gws[-1]))
        res["gw"], res["gw_bound"] = flat(gws), flat(bounds)
    return res


# ----------------------------------------------------------------------------------------------------------------- NGP heads
def mid_cin(h, sh16):
    """colour-net input of the density head: [half(SH_4(d)) | h1..h15 | 0], [B, 32]"""
    return np.concatenate([sh16, h[:, 1:16], np.zeros((len(h), 1))], 1)


def mid2_cin(h, sh16, enc):
    """two-encoder network: [half(SH_4(d)) | h1..h15 | enc | 0], [B, 64]; enc level-major [16, B, 2] -> columns 31 + 2 l + c"""
    return np.concatenate([sh16, h[:, 1:16], enc.transpose(1, 0, 2).reshape(len(h), 32), np.zeros((len(h), 1))], 1)


def sigma_with_tolerance(h0):
    """sigma = exp(h0) in float64, and the relative tolerance of an fp32 evaluation: the statement in float32 against float64 gives
    the format's own error e32 on these inputs; 4 x the largest relative e32 plus 2^-22"""
    ref = np.exp(np.asarray(h0, np.float64))
    e32 = np.abs(np.exp(np.asarray(h0, np.float32)).astype(np.float64) - ref) / ref
    return ref, 4 * float(e32.max()) + 2.0 ** -22


def mid_grad_h0(d_sigma, h0):
    """d_h[:, 0] = d_sigma exp(clamp(h0, -15, 15)) (unrounded)"""
    return np.asarray(d_sigma, np.float64) * np.exp(np.clip(np.asarray(h0, np.float64), -15.0, 15.0))


def mid_grad_routed(d_cin):
    """d_h[:, 1:16] = d_cin[:, 16:31]"""
    return d_cin[:, 16:31]


def mid2_grad_enc(d_cin):
    """d_enc [16, B, 2] = d_cin[:, 31:63]"""
    return d_cin[:, 31:63].reshape(len(d_cin), 16, 2).transpose(1, 0, 2)


def rgb_forward(out):
    """rgb = sigmoid(out[:, :3]) (unrounded; the kernel rounds it to binary16 and widens to fp32)"""
    return 1.0 / (1.0 + np.exp(-np.asarray(out, np.float64)[:, :3]))


def rgb_backward(d_rgb, rgb):
    """d_out[:, :3] = half(d_rgb) y (1 - y) (unrounded); columns 3..15 are zero"""
    y = np.asarray(rgb, np.float64)
    return h16(d_rgb) * (y * (1.0 - y))
