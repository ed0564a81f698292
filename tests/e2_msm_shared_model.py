"""Python model of vpin_e2_msm_shared: many linear combinations on E2 whose sums share their scalar vectors,

    sum[s] = sum over t < n_terms of  r[vec[s]][t] * P[base[s] + off[pat[s]][t]]        (a negative off entry: no term)

over enc_conv_model's groups (POINTS: affine points; LOGS: discrete logarithms to the base G), the layers' random-linear-
combination sums written as instances of it, and the device's digit recoding restated: signed 3-bit windows (Booth), digit w of a
scalar r is  -4 b[3w+2] + 2 b[3w+1] + b[3w] + b[3w-1]  with b[-1] = 0, a value in -4 .. 4 that depends on four bits alone: no carry
runs between the windows.  ceil((scalar_bits + 1) / 3) windows cover a scalar below 2^scalar_bits."""
import enc_conv_model as EM

WINDOW = 3


def msm_shared(grp, r, points, off, vec, pat, base):
    """r: n_vec lists of n_terms ints; points: group elements; off: n_pat lists of n_terms ints; vec, pat, base: one per sum"""
    out = []
    for v, p, b in zip(vec, pat, base):
        acc = grp.identity
        for t, o in enumerate(off[p]):
            if o >= 0:
                acc = grp.add(acc, grp.mul(r[v][t], points[b + o]))
        out.append(acc)
    return out


def n_windows(scalar_bits):
    return (scalar_bits + 1 + WINDOW - 1) // WINDOW


def booth_digit(r, w):
    """digit w of r, from the four bits 3w - 1 .. 3w + 2"""
    v = ((r << 1) >> (WINDOW * w)) & 0xF
    return ((v & 7) + 1) // 2 - (4 if v & 8 else 0)


def recode(r, scalar_bits):
    assert 0 <= r < (1 << scalar_bits)
    return [booth_digit(r, w) for w in range(n_windows(scalar_bits))]


def value(digits):
    return sum(d << (WINDOW * w) for w, d in enumerate(digits))


def edge_values(scalar_bits):
    """0, 1, and 2^k - 1, 2^k, 2^k + 1 at every window edge k = 3w and at the neighbouring bits, cut to scalar_bits, plus the
    largest scalar"""
    out = {0, 1, (1 << scalar_bits) - 1}
    for w in range(n_windows(scalar_bits) + 1):
        for k in (WINDOW * w - 1, WINDOW * w, WINDOW * w + 1):
            if k >= 0:
                out.update(v for v in ((1 << k) - 1, 1 << k, (1 << k) + 1) if v < (1 << scalar_bits))
    return sorted(out)


def window_offsets(H, W, fh, fw, pad, stride):
    """off[k][t]: the index inside its plane of tap k of output t's window, -1 in the padding; then one row off[taps][t] = t"""
    oh, ow = EM.out_dims(H, W, fh, fw, pad, stride)
    off = []
    for k in range(fh * fw):
        row = []
        for t in range(oh * ow):
            r, c = (t // ow) * stride + k // fw - pad, (t % ow) * stride + k % fw - pad
            row.append(r * W + c if 0 <= r < H and 0 <= c < W else -1)
        off.append(row)
    off.append(list(range(oh * ow)))
    return off


def conv_instance(planes, outs, H, W, fh, fw, pad, stride):
    """vpin_enc_conv2d's sums: per plane p the taps + 1 sums B'[p][0 .. taps) and the left side, all over the vector r[p].
    Returns (points, off, vec, pat, base): the points are the planes and then the outputs"""
    taps, per, n_terms = fh * fw, H * W, len(outs[0])
    points = [v for pl in planes for v in pl] + [v for o in outs for v in o]
    vec, pat, base = [], [], []
    for p in range(len(planes)):
        for k in range(taps + 1):
            vec.append(p)
            pat.append(k)
            base.append(p * per if k < taps else len(planes) * per + p * n_terms)
    return points, window_offsets(H, W, fh, fw, pad, stride), vec, pat, base


def convmc_instance(planes, outs, C, n_out, rows, H, W, fh, fw, pad, stride):
    """vpin_enc_conv2d_mc's sums: per pair q = (g, o) the chain over its connected channels (rows[o]) and taps, then the left
    side, all over r[q].  Returns (points, off, vec, pat, base)"""
    taps, per, n_terms = fh * fw, H * W, len(outs[0])
    points = [v for pl in planes for v in pl] + [v for o in outs for v in o]
    vec, pat, base = [], [], []
    for q in range(len(outs)):
        g, o = q // n_out, q % n_out
        for c in rows[o]:
            for k in range(taps):
                vec.append(q)
                pat.append(k)
                base.append((g * C + c) * per)
        vec.append(q)
        pat.append(taps)
        base.append(len(planes) * per + q * n_terms)
    return points, window_offsets(H, W, fh, fw, pad, stride), vec, pat, base
