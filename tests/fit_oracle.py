"""The comparison of a device Parzen mixture with the oracle's, shared by the
plan-level fit tests (test_gpu_fit_params.py, test_gpu_fit_tiers.py)."""
import numpy as np

from oracle import tpe_oracle as O


def assert_mixture_bit_exact(got, tobs, prior_weight, prior_mu, prior_sigma, lf, log_family, msg,
                             ref=None):
    """``got`` = plan.mixture(hp, side) against O.parzen_fit (stable ties) of
    the side's transformed observations ``tobs`` (tid order): mu, sigma and w
    equal bit for bit.  ``ref``: that fit when the caller has it already.

    A log family (loguniform, qloguniform, ...) is fitted on log(x), which the
    device takes itself: its log and numpy's are both within an ulp of the
    true one and differ in the last bit for a small share of the values.  So
    there the device's sorted means must pair with the oracle's within one ulp
    of each -- the same observations on each side, in the same order, the
    prior at the same place and exact -- and the oracle's fit of the device's
    own logarithms (taken from those means) must then equal the device's bit
    for bit."""
    w, mu, sg = got
    pw, pm, ps = prior_weight, prior_mu, prior_sigma
    if log_family:
        with np.errstate(all='ignore'):
            _, mu_o, _, order, pos = O.parzen_fit(tobs, pw, pm, ps, lf=lf, kind='stable',
                                                  return_order=True)
        off = np.abs(mu - mu_o)
        assert (off <= np.spacing(np.abs(mu_o))).all(), msg + 'log(x) beyond an ulp'
        assert mu[pos] == pm
        print('%s: %d of %d means differ from numpy\'s log in the last bit'
              % (msg, int((off > 0).sum()), mu.size))
        dev = np.array(tobs, dtype=np.float64)
        if dev.size:
            dev[np.arange(dev.size) if order is None else order] = np.delete(mu, pos)
        with np.errstate(all='ignore'):
            ref = O.parzen_fit(dev, pw, pm, ps, lf=lf, kind='stable')
    elif ref is None:
        with np.errstate(all='ignore'):
            ref = O.parzen_fit(tobs, pw, pm, ps, lf=lf, kind='stable')
    np.testing.assert_array_equal(mu, ref[1], err_msg=msg + 'mu')
    np.testing.assert_array_equal(sg, ref[2], err_msg=msg + 'sigma')
    np.testing.assert_array_equal(w, ref[0], err_msg=msg + 'w')
