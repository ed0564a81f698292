"""Python model of the encrypted fully connected layer with its random-linear-combination (RLC) check and of the encrypted
average-pooling layer: FCLayer (flag 1) with the type-1 branch of rLCL / rLCR, and myAvgPool2d (type1 = 1, flag = 1) of
src/LeNet/Server.py.  Both are checked against recorded runs of the reference's own functions: tests/golden/layer_pins.json
(tests/golden/make_layer_pins.py), compared in tests/test_layer_pins.py.
Generic over the group it computes in, like enc_conv_model: POINTS (the literal one) or LOGS (discrete logarithms)."""
import gadgets_model as GM
from enc_conv_model import G, ORDER, POINTS, LOGS, ShapeError, VerifyError, log_point, prf, synthetic_logs  # noqa: F401

_base_table = []  # _base_table[i][d] = d * 16^i * G


def _add(P1, P2):
    """gadgets_model.e2_add with Python's modular inverse in place of the power x^(q-2)"""
    if P1 is None or P2 is None:
        return P2 if P1 is None else P1
    (x1, y1), (x2, y2) = P1, P2
    if x1 == x2:
        if (y1 + y2) % GM.Q == 0:
            return None
        lam = (3 * x1 * x1 + GM.E2_A) * pow(2 * y1, -1, GM.Q) % GM.Q
    else:
        lam = (y2 - y1) * pow(x2 - x1, -1, GM.Q) % GM.Q
    x3 = (lam * lam - x1 - x2) % GM.Q
    return x3, (lam * (x1 - x3) - y1) % GM.Q


def base_point(k):
    """log_point(k) through a fixed-base table of 4-bit windows: at most 64 additions per point instead of ~380 with a power
    each, for the shapes whose lists hold hundreds of points (tests/test_enc_fc_model.py checks it against log_point)"""
    if not _base_table:
        B = G
        for _ in range(64):
            row = [None]
            for _ in range(15):
                row.append(_add(row[-1], B))
            _base_table.append(row)
            B = _add(row[15], B)
    k %= ORDER
    acc = None
    for i in range(64):
        acc = _add(acc, _base_table[i][(k >> (4 * i)) & 15])
    return acc


def fc(grp, rows, K, W, N, biases, keys, prf_bytes):
    """rows: P lists of K group elements; W[k][j]: K x N ints below 2^32; biases: P lists of N elements (the identity allowed);
    keys: one per row.  Returns dict(out = P lists of N elements, mults = [(s_k, X[k])], adds = per row the N pairs
    (C[j], bias[j]) and then the K - 1 pairs (acc, T_k) -- an identity second operand is what the witness writes as rz = 1 --,
    left = P elements)."""
    res = dict(out=[], mults=[], adds=[], left=[])
    for X, bias, key in zip(rows, biases, keys):
        assert len(X) == K and len(bias) == N and len(W) == K and all(len(w) == N for w in W)
        C = []
        for j in range(N):
            acc = grp.identity
            for k in range(K):
                acc = grp.add(acc, grp.mul(W[k][j], X[k]))
            C.append(acc)
        out = []
        for j in range(N):
            if C[j] == grp.identity:
                raise ShapeError(f"C[{j}] is the identity")
            res["adds"].append((C[j], bias[j]))
            out.append(grp.add(C[j], bias[j]))
        r = [prf(key, j, prf_bytes) for j in range(N)]
        left = grp.identity
        for j in range(N):
            left = grp.add(left, grp.mul(r[j], C[j]))
        s = [sum(r[j] * W[k][j] for j in range(N)) for k in range(K)]
        if max(s) >= 1 << 128:
            raise ShapeError("a folded weight does not fit 128 bits")
        acc = grp.identity
        T = []
        for k in range(K):
            if X[k] == grp.identity:
                raise ShapeError(f"X[{k}] is the identity")
            res["mults"].append((s[k], X[k]))
            T.append(grp.mul(s[k], X[k]))
        for k in range(K):
            if k == 0:
                acc = T[0]
                continue
            if acc == grp.identity:
                raise ShapeError(f"the accumulator before T_{k} is the identity")
            res["adds"].append((acc, T[k]))
            acc = grp.add(acc, T[k])
        if acc != left:
            raise VerifyError("sum_k s_k * X[k] != sum_j r_j * C[j]")
        res["out"].append(out)
        res["left"].append(left)
    return res


def pool_dims(H, W, k, stride):
    return (H - k) // stride + 1, (W - k) // stride + 1


def avgpool(grp, planes, H, W, k, stride, scale):
    """planes: P lists of H * W elements.  Returns dict(out = P lists of oh * ow elements scale * (window sum),
    adds = [(acc, e_m)] per output the k * k - 1 running additions, the window taken row-major)."""
    oh, ow = pool_dims(H, W, k, stride)
    res = dict(out=[], adds=[])
    for plane in planes:
        assert len(plane) == H * W
        out = []
        for i in range(oh):
            for j in range(ow):
                win = [plane[(i * stride + ii) * W + j * stride + jj] for ii in range(k) for jj in range(k)]
                acc = win[0]
                for m in range(1, k * k):
                    if acc == grp.identity:
                        raise ShapeError(f"the accumulator of output ({i}, {j}) before element {m} is the identity")
                    res["adds"].append((acc, win[m]))
                    acc = grp.add(acc, win[m])
                out.append(grp.mul(scale, acc))
        res["out"].append(out)
    return res
