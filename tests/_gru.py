"""NumPy oracle of the GRU recurrence, float64 unless asked for fp32 (test helper, not collected).

PyTorch nn.GRU semantics, gate order r, z, n, zero initial state.  The caller supplies the
time-parallel part xproj = x W_ih^T + b_ih + [b_hr, b_hz, 0] (B, T, 3H):

    a_t = W_hh h_{t-1};  r = sigmoid(xproj_r + a_r);  z = sigmoid(xproj_z + a_z)
    q = a_n + b_hn;  n = tanh(xproj_n + r q);  h_t = (1 - z) n + z h_{t-1}

gates (B, T, 4H) = [r, z, n, q].  Backward, t = T-1 .. 0, carry_T = 0:

    d = dh_t + carry_{t+1};  dn_pre = d (1 - z)(1 - n^2);  dz_pre = d (h_{t-1} - n) z (1 - z)
    dr_pre = dn_pre q r (1 - r);  carry_t = d z + W_hh^T [dr_pre, dz_pre, dn_pre r]
    dgates_t = [dr_pre, dz_pre, dn_pre, dn_pre r]                                  (4H)

gru_param_grads forms what the autograd formula forms from dgates: d xproj, dW_hh, db_hn.
"""
from __future__ import annotations

import numpy as np


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def gru_forward(xproj, w_hh, b_hn, dtype=np.float64, hook=None):
    """-> h (B, T, H), gates (B, T, 4H); every array and operation of the run in `dtype` (np.float32:
    genuine fp32 arithmetic).  hook("h_prev", t, h_{t-1}, h) may replace the operand of step t's
    recurrent product (tests/test_recurrence_bite.py plants defects through it)."""
    xproj, w_hh, b_hn = (np.asarray(v, dtype) for v in (xproj, w_hh, b_hn))
    B, T, H3 = xproj.shape
    H = H3 // 3
    h = np.zeros((B, T, H), dtype)
    gates = np.zeros((B, T, 4 * H), dtype)
    prev = np.zeros((B, H), dtype)
    for t in range(T):
        a = (prev if hook is None else hook("h_prev", t, prev, h)) @ w_hh.T
        r = _sigmoid(xproj[:, t, :H] + a[:, :H])
        z = _sigmoid(xproj[:, t, H:2 * H] + a[:, H:2 * H])
        q = a[:, 2 * H:] + b_hn
        n = np.tanh(xproj[:, t, 2 * H:] + r * q)
        prev = (1.0 - z) * n + z * prev
        h[:, t] = prev
        gates[:, t] = np.concatenate((r, z, n, q), axis=1)
    return h, gates


def gru_backward(w_hh, h, gates, dh, dtype=np.float64, hook=None):
    """-> dgates (B, T, 4H) = [dr_pre, dz_pre, dn_pre, dn_pre * r], in `dtype` throughout.
    hook("carry", t, carry_t, dgh_t, w_hh) may replace what step t hands to step t - 1."""
    w_hh, h, gates, dh = (np.asarray(v, dtype) for v in (w_hh, h, gates, dh))
    B, T, H = h.shape
    dgates = np.zeros((B, T, 4 * H), dtype)
    carry = np.zeros((B, H), dtype)
    for t in range(T - 1, -1, -1):
        r, z, n, q = (gates[:, t, i * H:(i + 1) * H] for i in range(4))
        prev = h[:, t - 1] if t > 0 else np.zeros((B, H), dtype)
        d = dh[:, t] + carry
        dn = d * (1.0 - z) * (1.0 - n * n)
        dz = d * (prev - n) * z * (1.0 - z)
        dr = dn * q * r * (1.0 - r)
        dgh = np.concatenate((dr, dz, dn * r), axis=1)
        carry = d * z + dgh @ w_hh
        if hook is not None:
            carry = hook("carry", t, carry, dgh, w_hh)
        dgates[:, t] = np.concatenate((dr, dz, dn, dn * r), axis=1)
    return dgates


def gru_param_grads(h, dgates):
    """-> d xproj (B, T, 3H), dW_hh (3H, H), db_hn (H) from the saved h and dgates."""
    h, dgates = np.asarray(h, np.float64), np.asarray(dgates, np.float64)
    B, T, H = h.shape
    dxproj = dgates[..., :3 * H]
    dgh = np.concatenate((dgates[..., :2 * H], dgates[..., 3 * H:]), axis=-1)
    dw_hh = dgh[:, 1:].reshape(-1, 3 * H).T @ h[:, :-1].reshape(-1, H)
    db_hn = dgh[..., 2 * H:].reshape(-1, H).sum(0)
    return dxproj, dw_hh, db_hn
