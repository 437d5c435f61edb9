"""Shared by tests/test_simulate_host.py and tests/test_hip_synphot.py: the survey of golden G20 rebuilt through the array loaders,
and small synthetic surveys for the shapes the fixture does not hold."""
import numpy as np

from conftest import load_golden

_cache = {}


def g20():
    if 'g' not in _cache:
        g = load_golden('g20_synphot')
        _cache['g'] = {k: g[k] for k in g.files}
    return _cache['g']


def golden_survey():
    """a fresh MockSurvey holding G20's 5 filters and 4 templates; the fourth template is cut to 3000-9000 A by hand after
    loading, as the maker cut it"""
    from frankenz_amd import simulate
    g = g20()
    ms = simulate.MockSurvey()
    nf, nt = len(g['f_names']), len(g['t_names'])
    ms.set_filters([str(n) for n in g['f_names']], [g['f%d_wave' % i] for i in range(nf)], [g['f%d_trans' % i] for i in range(nf)],
                   g['f_depth'])
    ms.set_refmag('r')
    ms.set_templates([str(n) for n in g['t_names']], [str(t) for t in g['t_types']], [g['t%d_wave' % i] for i in range(nt)],
                     [g['t%d_flambda_raw' % i] for i in range(nt)])
    return ms


def cut_last_template(ms):
    t, keep = ms.templates[3], g20()['t3_keep']
    for k in ('wavelength', 'frequency', 'flambda', 'fnu'):
        t[k] = t[k][keep]
    return ms


def restore_state(g, tag):
    rs = np.random.RandomState()
    pos = g[tag + '_pos']
    rs.set_state(('MT19937', g[tag + '_keys'], int(pos[0]), int(pos[1]), float(g[tag + '_gauss'])))
    return rs


def same_state(rs, g, tag):
    name, keys, pos, has_gauss, cached = rs.get_state()
    return (np.array_equal(keys, g[tag + '_keys']) and [pos, has_gauss] == [int(v) for v in g[tag + '_pos']] and
            cached == float(g[tag + '_gauss']))


def synthetic_survey(filter_sizes, template_sizes, seed=0, tmpl_range=(800., 30000.)):
    """a MockSurvey of smooth bumps: filters of the given point counts spread over 2500-11000 A (the last point count may be 2),
    templates of the given point counts on a log grid over ``tmpl_range`` with a break and a few lines"""
    from frankenz_amd import simulate
    rs = np.random.RandomState(seed)
    ms = simulate.MockSurvey()
    names, waves, trans = [], [], []
    for i, n in enumerate(filter_sizes):
        lo = 2500. + 8000. * i / max(1, len(filter_sizes))
        w = np.linspace(lo, lo + 900., n)
        tr = np.exp(-0.5 * ((w - w.mean()) / 250.)**2) + 0.01
        names.append('f%d' % i); waves.append(w); trans.append(tr)
    ms.set_filters(names, waves, trans, np.full(len(names), 25.))
    ms.set_refmag(0, mode='counter')
    tn, tt, tw, tf = [], [], [], []
    for i, n in enumerate(template_sizes):
        w = np.exp(np.linspace(np.log(tmpl_range[0]), np.log(tmpl_range[1]), n))
        fl = (w / 5000.)**(-1.5 + 0.7 * i) * (1. + 0.8 * (w > 4000.)) + 0.3 * np.exp(-0.5 * ((w - 6563.) / 30.)**2)
        fl *= 1. + 0.05 * rs.rand(n)
        tn.append('t%d' % i); tt.append('T%d' % (i % 3)); tw.append(w); tf.append(fl)
    ms.set_templates(tn, tt, tw, tf)
    return ms
