"""A model of the merge kernels' register list (merge_step / merge_peel in csrc/ansfm_merge64.hip.h) in plain Python: the
order in which the G * G sums are popped with full-length passes throughout against the order with the last G - 1 passes
shortened by one entry per step, for every G of every instantiated list length -- flat input (keys that tie), zeros and
list entries beyond G included.  It also checks the compile-time choice of which of e0 / e1 holds the current element in
each peeled step.  No GPU: this pins the argument, tests/test_merge_trim.py pins the kernel."""
import random
import struct

import pytest

HUGE = struct.unpack('<d', struct.pack('<Q', 0x7FE0000000000000))[0]


def pack(v, row, col):
    b = struct.unpack('<Q', struct.pack('<d', v))[0]
    b = (b & ~0x7FF) | ((col << 5) | row)
    return struct.unpack('<d', struct.pack('<Q', b))[0]


def dec(key):
    kb = struct.unpack('<Q', struct.pack('<d', key))[0] & 0xFFFFFFFF
    return kb & 31, (kb >> 5) & 63


def fetch(key, A, B):
    ci, cp = dec(key)
    return dict(ci=ci, np=cp + 1, ai=A[ci] if ci < len(A) else 0.0, bc=B[cp] if cp < len(B) else 0.0, bn=B[cp + 1] if cp + 1 < len(B) else 0.0)


def step(R, e, A, B, NP):
    x = pack(e['ai'] + e['bn'], e['ci'], e['np'])
    if NP == 1:
        R[0] = x; return None
    R[0] = min(x, R[1])
    en = fetch(R[0], A, B)
    mk = [max(x, R[k]) for k in range(1, NP - 1)]
    for j, k in enumerate(range(1, NP - 1)): R[k] = min(mk[j], R[k + 1])
    R[NP - 1] = max(x, R[NP - 1])
    return en


def run(A, B, G, NR, peel):
    Bx = list(B) + [HUGE]
    R = [pack(A[i] + Bx[0], i, 0) if i < G else HUGE for i in range(NR)]
    assert all(R[i] <= R[i + 1] for i in range(NR - 1))
    e = [fetch(R[0], A, Bx), None]; cur = 0; out = []

    def do(NP):
        nonlocal cur
        en = step(R, e[cur], A, Bx, NP)
        out.append((e[cur]['ci'], e[cur]['np'] - 1, e[cur]['ai'] + e[cur]['bc']))
        e[1 - cur] = en; cur = 1 - cur
    nloop = G * G - (G - 1) if peel else G * G
    for _ in range(nloop): do(NR)
    if peel:
        # the kernel hands the current element over in e1 when G and NR have the same parity; then body NP takes
        # e1 as current iff (NR - NP) odd -- check that this static choice names the current element
        phys = cur if ((G ^ NR) & 1) == 0 else 1 - cur       # after the optional swap, which slot holds it
        for NP in range(NR - 1, 0, -1):
            if NP < G:
                want = 1 if ((NR - NP) & 1) else 0
                assert want == phys, (G, NR, NP)
                do(NP); phys = 1 - phys
    return out


@pytest.mark.parametrize("NR", [8, 10, 16, 20, 32])
def test_peeled_passes_pop_the_same_order(NR):
    random.seed(NR)
    for G in range(1, NR + 1):
        for trial in range(6):
            flat = trial % 3 == 1
            A = sorted((1.0 + i * 1e-12 if flat else 10 ** random.uniform(-3, 2)) for i in range(G))
            B = sorted((2.0 + i * 1e-12 if flat else 10 ** random.uniform(-3, 2)) for i in range(G))
            if trial % 3 == 2:
                A[:G // 2] = [0.0] * (G // 2)
            full = run(A, B, G, NR, False)
            peeled = run(A, B, G, NR, True)
            assert full == peeled, (NR, G, trial)
            assert len(full) == G * G and len(set((r, c) for r, c, _ in full)) == G * G
