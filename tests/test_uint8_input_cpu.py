"""The 8-bit image form and the feeder, host side: the conversion table is `pil_to_tensor`'s arithmetic bit for bit, the shelf
readers return the same item in either form, malformed 8-bit tensors are refused before any device check, and ImageFeeder's
threading (order, bounded read-ahead, exceptions in place, clean shutdown) holds without a GPU (`device=None`)."""
import threading
import time

import pytest
import torch


def _bits(t):
    return t.contiguous().view(torch.int32)


def _pil(shape, seed, mode):
    from PIL import Image
    a = (torch.rand(*shape, generator=torch.Generator().manual_seed(seed)) * 256).clamp(max=255).to(torch.uint8)
    return Image.fromarray(a.numpy(), mode)


def _to_float(u):
    """What the device does, on the host: the table gather."""
    from cvpce_amd import ops
    return ops.uint8_to_float(u)


def test_table_is_pil_to_tensor_for_all_codes():
    from PIL import Image
    from cvpce_amd import datautils, ops
    codes = torch.arange(256, dtype=torch.uint8).view(16, 16)
    want = datautils.pil_to_tensor(Image.fromarray(codes.numpy(), 'L')).reshape(-1)
    table = ops.uint8_table()
    assert table.dtype == torch.float32 and table.shape == (256,)
    assert torch.equal(_bits(table), _bits(want))
    # the reason for the table: a multiplication by the reciprocal is NOT that arithmetic
    assert int((_bits(torch.arange(256, dtype=torch.float32) * torch.tensor(1 / 255, dtype=torch.float32)) != _bits(want)).sum()) > 100


@pytest.mark.parametrize('mode,shape', [('RGB', (37, 53, 3)), ('L', (29, 31)), ('RGBA', (16, 40, 4))])
def test_gather_of_pil_to_uint8_is_pil_to_tensor(mode, shape):
    from cvpce_amd import datautils, ops
    img = _pil(shape, 7, mode)
    u = datautils.pil_to_uint8(img)
    c = 1 if mode == 'L' else shape[2]
    assert u.dtype == torch.uint8 and u.is_contiguous() and tuple(u.shape) == (shape[0], shape[1], c)
    got = ops.uint8_table()[u.permute(2, 0, 1).to(torch.int64)]
    assert torch.equal(got, datautils.pil_to_tensor(img))
    if mode == 'RGB':
        f = ops.uint8_to_float(u)
        assert f.is_contiguous() and f.dtype == torch.float32 and torch.equal(_bits(f), _bits(datautils.pil_to_tensor(img)))
        assert torch.equal(ops.device_image(u, 'cpu'), f)
        same = datautils.pil_to_tensor(img)
        assert torch.equal(ops.device_image(same, 'cpu'), same)


def test_image_hw_on_both_forms():
    from cvpce_amd import datautils
    assert datautils.image_hw(torch.zeros(3, 40, 60)) == (40, 60)
    assert datautils.image_hw(torch.zeros(40, 60, 3, dtype=torch.uint8)) == (40, 60)
    assert datautils.image_hw(torch.zeros(1, 3, 3)) == (3, 3) and datautils.image_hw(torch.zeros(3, 7, 3, dtype=torch.uint8)) == (3, 7)


def _same(a, b):
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.dtype == b.dtype and torch.equal(a, b)
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) == type(b) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if type(a).__module__.startswith('networkx'):
        return a is b or (sorted(a.nodes(data='label')) == sorted(b.nodes(data='label')) and sorted(a.edges(data='dir')) == sorted(b.edges(data='dir')))
    return a == b


@pytest.fixture(scope='module')
def shelf_files(tmp_path_factory):
    """One tiny on-disk instance of every shelf dataset (the temporary-file style of tests/test_datasets_cpu.py)."""
    import json
    root = tmp_path_factory.mktemp('uint8_readers')
    # SKU-110K
    (root / 'sku').mkdir()
    _pil((40, 60, 3), 1, 'RGB').save(root / 'sku' / 'test_0.png')
    _pil((48, 36, 3), 2, 'RGB').save(root / 'sku' / 'test_1.png')
    (root / 'sku' / 'ann.csv').write_text('test_0.png,1,2,30,35,object,60,40\ntest_1.png,3,4,20,25,object,36,48\ntest_0.png,5,6,40,30,object,60,40\n')
    # GP baseline and GP-180 (+ planograms) share the store tree
    (root / 'gp' / 'store1' / 'images').mkdir(parents=True)
    _pil((50, 70, 3), 3, 'RGB').save(root / 'gp' / 'store1' / 'images' / 'store1_15.jpg', format='PNG')
    _pil((44, 52, 3), 4, 'RGB').save(root / 'gp' / 'store1' / 'images' / 'store1_16.jpg', format='PNG')
    (root / 'base.csv').write_text('name,x1,y1,x2,y2,cls\nstore1_15.jpg,1,2,30,35,0\nstore1_16.jpg,3,4,20,25,0\n')
    (root / 'ann').mkdir(); (root / 'plano').mkdir()
    for img_id in (15, 16):
        (root / 'ann' / f's1_{img_id}.csv').write_text('Food/Tea/1.jpg, 1, 2, 20, 30\nFood/Tea/2.jpg, 22, 2, 40, 30\n')
        graph = [{'ogg': j, 'n': -1, 's': -1, 'e': j + 1 if j < 1 else -1, 'w': j - 1, 'ne': -1, 'nw': -1, 'se': -1, 'sw': -1} for j in range(2)]
        objects = [{'width': 19, 'height': 28, 'img_path': f'Food/Tea/{j + 1}.jpg'} for j in range(2)]
        (root / 'plano' / f's1_{img_id}.json').write_text(json.dumps({'graph': graph, 'objects': objects}))
    # internal planogram set
    (root / 'internal').mkdir()
    _pil((42, 66, 3), 5, 'RGB').save(root / 'internal' / 'a.png')
    (root / 'internal' / 'a.json').write_text(json.dumps([{'code': '123', 'box': [0, 0, 10, 20]}, {'code': '456', 'box': [12, 0, 22, 20]}]))
    (root / 'internal' / 'index.json').write_text(json.dumps([{'image': 'a.png', 'planogram': 'a.json', 'correct': 1, 'facings': 2}]))
    return root


def _readers(root):
    from cvpce_amd import datautils
    return {
        'sku110k': lambda **kw: datautils.SKU110KDataset(str(root / 'sku'), str(root / 'sku' / 'ann.csv'), **kw),
        'gpbaseline': lambda **kw: datautils.GPBaselineDataset(str(root / 'gp'), str(root / 'base.csv'), **kw),
        'gp180': lambda **kw: datautils.GroceryProductsTestSet(str(root / 'gp'), str(root / 'ann'), **kw),
        'gp180_retinanet': lambda **kw: datautils.GroceryProductsTestSet(str(root / 'gp'), str(root / 'ann'), retinanet_annotations=True, **kw),
        'planograms': lambda **kw: datautils.PlanogramTestSet(str(root / 'gp'), str(root / 'ann'), str(root / 'plano'), **kw),
        'internal': lambda **kw: datautils.InternalPlanoSet(str(root / 'internal'), **kw),
    }


@pytest.mark.parametrize('name', ['sku110k', 'gpbaseline', 'gp180', 'gp180_retinanet', 'planograms', 'internal'])
def test_shelf_readers_in_uint8_form(shelf_files, name):
    make = _readers(shelf_files)[name]
    default, explicit, narrow = make(), make(image_format='float'), make(image_format='uint8')
    assert len(default) == len(narrow) >= 1
    for i in range(len(default)):
        want, same, got = default[i], explicit[i], narrow[i]
        assert want[0].dtype == torch.float32 and _same(tuple(want), tuple(same))
        u = got[0]
        h, w = want[0].shape[1:]
        assert u.dtype == torch.uint8 and tuple(u.shape) == (h, w, 3) and u.is_contiguous()
        assert torch.equal(_bits(_to_float(u)), _bits(want[0]))
        assert len(got) == len(want) and _same(tuple(want[1:]), tuple(got[1:]))
    with pytest.raises(ValueError):
        make(image_format='bytes')


@pytest.mark.parametrize('shape', [(3, 40, 60), (40, 60, 4)])
def test_malformed_uint8_is_a_type_error_before_the_device_check(shape):
    from cvpce_amd import production, synthetic
    bad = torch.zeros(shape, dtype=torch.uint8)
    model = synthetic.synthetic_gln(seed=0, detections_per_img=8)        # on the CPU: anything that got to the device check raises RuntimeError
    with pytest.raises(TypeError, match='uint8'):
        model([bad])
    with pytest.raises(TypeError, match='uint8'):
        model([torch.zeros(3, 40, 60), bad])
    pg = production.ProposalGenerator(model, device=torch.device('cpu'))
    with pytest.raises(TypeError, match='uint8'):
        pg.generate_proposals(bad)
    with pytest.raises(TypeError, match='uint8'):
        pg.generate_proposals_and_images(bad)
    # a well-formed 8-bit image gets as far as the device check
    with pytest.raises(RuntimeError):
        model([torch.zeros(40, 60, 3, dtype=torch.uint8)])


# ---- ImageFeeder without a device: the threading alone --------------------------------------------------------------
class _Sleepy:
    def __init__(self, n, fail_at=None):
        self.n, self.fail_at = n, fail_at
        self.lock = threading.Lock()
        self.started = 0
        self.threads = set()

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        with self.lock:
            self.started += 1
            self.threads.add(threading.get_ident())
        time.sleep((i % 5) / 1000)
        if i == self.fail_at:
            raise OSError(f'item {i} is broken')
        return torch.full((4, 5, 3), i, dtype=torch.uint8), {'i': i}


def test_feeder_keeps_order():
    from cvpce_amd.feeding import ImageFeeder
    data = _Sleepy(40)
    got = list(ImageFeeder(data, workers=4, device=None))
    assert [d['i'] for _, d in got] == list(range(40))
    assert all(not img.is_cuda and img.dtype == torch.uint8 and int(img[0, 0, 0]) == d['i'] for img, d in got)
    assert len(data.threads) > 1 and threading.get_ident() not in data.threads
    assert len(ImageFeeder(data, workers=4)) == 40


@pytest.mark.parametrize('workers,depth', [(2, 3), (4, None), (50, 1)])
def test_feeder_read_ahead_is_bounded(workers, depth):
    from cvpce_amd import feeding
    data = _Sleepy(60)
    feeder = feeding.ImageFeeder(data, workers=workers, depth=depth, device=None)
    assert feeder.workers == min(workers, 16)                     # capped: never sized by the machine's CPU count
    bound = feeder.workers + (depth if depth is not None else feeding.DEFAULT_DEPTH)
    worst = 0
    for yielded, _ in enumerate(feeder, start=1):
        with data.lock:
            worst = max(worst, data.started - yielded)
        time.sleep(0.002)                                          # a slow consumer: the readers run as far ahead as they may
    assert worst <= bound, (worst, bound)
    assert worst >= 1                                              # ... and they did run ahead


def test_feeder_raises_at_the_items_position():
    from cvpce_amd.feeding import ImageFeeder
    seen = []
    with pytest.raises(OSError, match='item 7'):
        for _, d in ImageFeeder(_Sleepy(20, fail_at=7), workers=4, device=None):
            seen.append(d['i'])
    assert seen == list(range(7))


def test_feeder_break_leaves_no_thread():
    from cvpce_amd.feeding import ImageFeeder
    before = threading.active_count()
    for n, _ in enumerate(ImageFeeder(_Sleepy(200), workers=8, device=None)):
        if n == 2:
            break
    deadline = time.time() + 1.0
    while threading.active_count() > before and time.time() < deadline:
        time.sleep(0.01)
    assert threading.active_count() == before
    # an explicitly closed iterator does the same
    it = iter(ImageFeeder(_Sleepy(200), workers=8, device=None))
    next(it); it.close()
    deadline = time.time() + 1.0
    while threading.active_count() > before and time.time() < deadline:
        time.sleep(0.01)
    assert threading.active_count() == before


def test_feeder_without_workers_reads_in_the_calling_thread():
    from cvpce_amd.feeding import ImageFeeder, feed
    data = _Sleepy(6)
    before = threading.active_count()
    worst = 0
    for yielded, (_, d) in enumerate(ImageFeeder(data, workers=0, device=None), start=1):
        worst = max(worst, data.started - yielded)
        assert threading.active_count() == before
    assert data.threads == {threading.get_ident()} and worst == 0 and d['i'] == 5
    # an iterable that cannot be indexed is read in the calling thread too, in order
    assert [int(x[0, 0, 0]) for x in ImageFeeder((torch.full((2, 2, 3), i, dtype=torch.uint8) for i in range(5)), workers=4)] == list(range(5))
    # what the evaluation functions do with num_workers
    assert feed(data, 0) is data and feed(data, None) is data and isinstance(feed(data, 3), ImageFeeder) and feed(data, 3).workers == 3
    f = ImageFeeder(data, workers=2)
    assert feed(f, 5) is f


def test_eval_functions_default_to_serial_reading():
    import inspect
    from cvpce_amd import classification_eval, detection_eval, proposals_eval
    for fn in (proposals_eval.evaluate_gln_sync, proposals_eval.evaluate_gln_async, proposals_eval.evaluate_gln,
               classification_eval.eval_dihe, detection_eval.evaluate_detections):
        assert inspect.signature(fn).parameters['num_workers'].default == 0, fn.__name__
