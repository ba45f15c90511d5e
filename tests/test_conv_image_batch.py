"""conv.prepare_images / finish_images and the layers' pick-up (wc_gan_amd/conv.py, "a pass's weight images in one launch") as host logic:
the library and the batched build are stubbed, so what runs here is the log, its key and the rule by which a layer takes a prepared image.
A per-layer build returns its (image, scale) tensors, a batched one the token ('batch', request index, geometry index)."""
import pytest
import torch
import torch.nn as nn


class _Site(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = nn.Conv2d(4, 4, 3)


class _Root(nn.Module):
    def __init__(self):
        super().__init__()
        self.a, self.b = _Site(), _Site()


def _Geom():
    from wc_gan_amd import _lib
    return _lib.ConvGeom()


@pytest.fixture
def C(monkeypatch):
    """conv with the per-layer entries and build_images replaced by counters"""
    from wc_gan_amd import conv
    calls = dict(single=0, pair=0, batch=[])

    class _FakeLib:
        def wc_conv_weights_bytes(self, g):
            return 16

        def wc_conv_weights_f32(self, *a):
            calls['single'] += 1
            return 0

        def wc_conv_weights_pair_f32(self, *a):
            calls['pair'] += 1
            return 0

    def build(requests):
        calls['batch'].append([(w, geoms) for w, geoms in requests])
        return [tuple(('batch', i, j) for j in range(len(geoms))) for i, (w, geoms) in enumerate(requests)]

    monkeypatch.setattr(conv._lib, 'load', lambda: _FakeLib())
    monkeypatch.setattr(conv, '_stream', lambda: None)
    monkeypatch.setattr(conv, '_ptr', lambda t: None)
    monkeypatch.setattr(conv, 'build_images', build)
    monkeypatch.setattr(conv, 'BATCH_IMAGES', True)
    conv.calls = calls
    yield conv
    del conv.calls
    conv._recording = conv._prepared = None


def _is_batch(r):
    return isinstance(r, tuple) and len(r) == 3 and isinstance(r[0], str) and r[0] == 'batch'


def _pass(C, root, key, requests):
    """one pass: requests = [(site, weight, geometries)]; -> what each request got"""
    C.prepare_images(root, key)
    try:
        out = []
        for site, w, geoms in requests:
            if len(geoms) == 2:
                out.append(C.weight_image_pair(w, geoms[0], geoms[1], site=site))
            else:
                out.append(C.weight_image(w, *geoms[0], site=site))
        return out
    finally:
        C.finish_images(root)


def test_a_pass_is_logged_once_and_batched_from_the_second_on(C):
    root = _Root()
    g1, g2, g3 = (_Geom(), 1, 0), (_Geom(), 0, 1), (_Geom(), 1, 0)
    reqs = [(root.a, root.a.conv.weight, (g1, g2)), (root.b, root.b.conv.weight, (g3,))]
    first = _pass(C, root, 'k', reqs)
    assert C.calls == dict(single=1, pair=1, batch=[]) and not any(_is_batch(r) or _is_batch(r[0]) for r in first)
    for n in (1, 2):
        got = _pass(C, root, 'k', reqs)
        assert C.calls['single'] == 1 and C.calls['pair'] == 1 and len(C.calls['batch']) == n
        assert got == [(('batch', 0, 0), ('batch', 0, 1)), ('batch', 1, 0)]
    # the build saw the layers' own weights and the logged geometries, pair and single
    (w0, geoms0), (w1, geoms1) = C.calls['batch'][-1]
    assert w0 is root.a.conv.weight and w1 is root.b.conv.weight
    assert geoms0 == (g1, g2) and geoms1 == (g3,)


def test_another_key_gives_no_batch_and_has_a_log_of_its_own(C):
    root = _Root()
    g = (_Geom(), 1, 0)
    reqs = [(root.a, root.a.conv.weight, (g,))]
    _pass(C, root, 'k', reqs)
    _pass(C, root, 'k', reqs)
    assert C.calls['single'] == 1 and len(C.calls['batch']) == 1
    got = _pass(C, root, 'other', reqs)                     # first pass under the other key: the layer builds
    assert C.calls['single'] == 2 and len(C.calls['batch']) == 1 and not _is_batch(got[0])
    assert _is_batch(_pass(C, root, 'other', reqs)[0]) and _is_batch(_pass(C, root, 'k', reqs)[0])
    assert C.calls['single'] == 2 and len(C.calls['batch']) == 3


def test_the_key_tells_passes_apart_by_shape_grad_mode_training_and_parameter_flags(C):
    root = _Root()
    x = torch.zeros(2, 3)
    k0 = C.pass_key(root, x)
    assert k0 == C.pass_key(root, torch.ones(2, 3))
    assert k0 != C.pass_key(root, torch.zeros(4, 3))
    assert k0 != C.pass_key(root, torch.zeros(2, 3, requires_grad=True))
    with torch.no_grad():
        assert k0 != C.pass_key(root, x)
    root.eval()
    assert k0 != C.pass_key(root, x)
    root.train()
    root.b.conv.weight.requires_grad_(False)                # what g_step does to the critic
    assert k0 != C.pass_key(root, x)
    root.b.conv.weight.requires_grad_(True)
    assert k0 == C.pass_key(root, x)


def test_another_tensor_object_or_geometry_falls_back(C):
    root = _Root()
    g = (_Geom(), 1, 0)
    w = root.a.conv.weight
    _pass(C, root, 'k', [(root.a, w, (g,))])
    assert C.calls['single'] == 1
    # an equal tensor that is not the one the image was built from
    got = _pass(C, root, 'k', [(root.a, w.detach().clone(), (g,))])
    assert not _is_batch(got[0]) and C.calls['single'] == 2 and len(C.calls['batch']) == 1
    # (the log did not foresee that pass: it is dropped, and written again by the next one)
    assert 'k' not in root._wc_image_logs
    _pass(C, root, 'k', [(root.a, w, (g,))])
    assert C.calls['single'] == 3 and len(C.calls['batch']) == 1
    # an equal geometry that is another object (another plan: another input size), and other axes
    same = _Geom()
    for other in ((same, 1, 0), (g[0], 0, 1)):
        C.prepare_images(root, 'k')
        n = C.calls['single']
        assert not _is_batch(C.weight_image(w, *other, site=root.a)) and C.calls['single'] == n + 1
        assert _is_batch(C.weight_image(w, *g, site=root.a)) and C.calls['single'] == n + 1      # the prepared one is still there for its own request
        C._prepared[2] = False
        C.finish_images(root)
    # a single request does not take half a pair
    C.prepare_images(root, 'k')
    assert not _is_batch(C.weight_image_pair(w, g, (same, 0, 1), site=root.a)[0])
    C.finish_images(root)


def test_a_record_is_taken_once_and_none_outlives_its_pass(C):
    root = _Root()
    g = (_Geom(), 1, 0)
    w = root.a.conv.weight
    _pass(C, root, 'k', [(root.a, w, (g,))])
    C.prepare_images(root, 'k')
    assert root.a._wc_images and root.a._wc_images[0][0] is w
    assert _is_batch(C.weight_image(w, *g, site=root.a))
    assert not root.a._wc_images                            # cleared on pick-up ...
    n = C.calls['single']
    assert not _is_batch(C.weight_image(w, *g, site=root.a)) and C.calls['single'] == n + 1     # ... so a second request builds
    C.finish_images(root)
    # a prepared image nobody takes is gone when the pass ends
    _pass(C, root, 'k', [(root.a, w, (g,))])
    C.prepare_images(root, 'k')
    assert root.a._wc_images
    C.finish_images(root)
    assert root.a._wc_images is None and root._wc_image_sites == ()
    n = C.calls['single']
    assert not _is_batch(C.weight_image(w, *g, site=root.a)) and C.calls['single'] == n + 1     # outside a pass: the layer's own
    # a pass that never ended (an exception in a layer) leaves nothing to the next one either
    _pass(C, root, 'k', [(root.a, w, (g,))])
    _pass(C, root, 'k', [(root.a, w, (g,))])
    C.prepare_images(root, 'k')
    assert root.a._wc_images
    C.prepare_images(root, 'other')
    assert root.a._wc_images is None


def test_the_switch_and_requests_without_a_layer(C, monkeypatch):
    root = _Root()
    g = (_Geom(), 1, 0)
    w = root.a.conv.weight
    monkeypatch.setattr(C, 'BATCH_IMAGES', False)
    for _ in range(3):
        assert not _is_batch(_pass(C, root, 'k', [(root.a, w, (g,))])[0])
    assert C.calls['single'] == 3 and C.calls['batch'] == [] and not root.__dict__.get('_wc_image_logs')
    monkeypatch.setattr(C, 'BATCH_IMAGES', True)
    C.prepare_images(root, 'k')
    C.weight_image(w, *g)                                   # no layer named: neither logged nor looked up
    C.finish_images(root)
    assert root._wc_image_logs['k'] == []
    _pass(C, root, 'k', [])
    assert C.calls['batch'] == []                           # an empty log launches nothing


def test_a_spectral_layer_is_prepared_from_the_weight_that_waits_for_it():
    from wc_gan_amd import conv as C
    site = _Site()
    conv = site.conv
    conv.normalized_weight = lambda: None
    assert C._own_weight(site) is None                      # nothing prepared: the layer normalises, and builds, on its own
    w_sn = torch.zeros(4, 4, 3, 3)
    conv._w_ready = (w_sn, conv.weight._version, conv.training)
    assert C._own_weight(site) is w_sn and conv._w_ready is not None     # looked at, not taken
    conv._w_ready = (w_sn, conv.weight._version + 1, conv.training)
    assert C._own_weight(site) is None
    plain = _Site()
    assert C._own_weight(plain) is plain.conv.weight
    assert C._own_weight(nn.ReLU()) is None
