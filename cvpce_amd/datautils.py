"""Counterpart of /root/reference/cvpce/datautils.py: the hot-path member (`resize_for_classification`, on the GPU) and the
host-side dataset readers of the eval commands (below)."""
import torch


CLASSIFICATION_IMAGE_SIZE = 256


def resize_for_classification(img):
    """datautils.py:234-239: pad (3,h,w) to a square with 0.5 (top-left anchored), bilinear -> 256x256.

    Runs the K9 HIP gather kernel (the whole image is the crop box).  An 8-bit (h,w,3) image is read as bytes (ops.U8_KERNELS) or
    converted on the device first."""
    from . import ops          # the only kernel calls in this module: the readers below are host-only
    ops.check_image_form(img)
    if not img.is_cuda:
        raise RuntimeError('resize_for_classification runs on an MI355X (HIP) device only (no CPU fallback)')
    h, w = image_hw(img)
    box = torch.tensor([[0.0, 0.0, float(w), float(h)]], device=img.device)
    return ops.crop_resize(ops.input_image(img, img.device), box, CLASSIFICATION_IMAGE_SIZE, mode=0)[0]


def image_hw(img):
    """(H, W) of a shelf image in either form: float (3,H,W) or uint8 (H,W,3)."""
    if img.dtype == torch.uint8:
        return int(img.shape[0]), int(img.shape[1])
    return int(img.shape[-2]), int(img.shape[-1])


# ---------------------------------------------------------------------------------------------------------------------
# Gaussian target maps (datautils.py:18-85), rendered on the GPU by csrc/gaussians.hip under the rule of DESIGN.md 4c.  The
# reference's generate methods are closures and its join methods functions that run per box on the host; here both are
# small descriptors the kernel is told about, under the reference's names and numeric defaults.
# ---------------------------------------------------------------------------------------------------------------------
class GenerateMethod:
    """What `generate_via_*` returns: the method's name, its three kernel parameters and, for the kant method, (size, sigma)."""

    def __init__(self, name, params, table=None):
        self.name, self.params, self.table = name, tuple(float(p) for p in params), table

    def __repr__(self):
        return f'GenerateMethod({self.name!r}, {self.params}, table={self.table})'


class JoinMethod:
    def __init__(self, name):
        self.name = name

    def __repr__(self):
        return f'JoinMethod({self.name!r})'


def _scalar_only(value, func_name, scalar_name, default_form):
    if value is not None:
        raise TypeError(f'{func_name} is a callable in the reference ({default_form}); on the GPU it is the scalar of that form: '
                        f'pass {scalar_name}=<number> instead')


def generate_via_multivariate_normal(peak=1, variance_func=None, variance_scale=0.5):
    """datautils.py:27-37 with `variance_func = lambda a: (a * variance_scale) ** 2` (the reference's default: a / 2)."""
    _scalar_only(variance_func, 'variance_func', 'variance_scale', 'lambda a: (a/2)**2')
    if not variance_scale > 0:
        raise ValueError('variance_scale must be positive')
    return GenerateMethod('multivariate_normal', (peak, variance_scale, 0))


def generate_via_kant_method(size=120, sigma=40):
    """datautils.py:39-54: a size x size table resampled to every clipped box."""
    if int(size) != size or int(sigma) != sigma or not 1 <= size <= 4096 or sigma < 1:
        raise ValueError('size is an integer in [1, 4096], sigma a positive integer')
    return GenerateMethod('kant_method', (0, 0, 0), table=(int(size), int(sigma)))


def generate_via_simple_and_scaled(minimum=-1, maximum=1, sigma_func=None, sigma_divisor=6):
    """datautils.py:56-63 with `sigma_func = lambda c: c / sigma_divisor` (the reference's default: c / 6)."""
    _scalar_only(sigma_func, 'sigma_func', 'sigma_divisor', 'lambda c: c / 6')
    if not sigma_divisor > 0:
        raise ValueError('sigma_divisor must be positive')
    return GenerateMethod('simple_and_scaled', (minimum, maximum, sigma_divisor))


join_via_max = JoinMethod('max')
join_via_addition = JoinMethod('addition')
join_via_replacement = JoinMethod('replacement')


def generate_gaussians(w, h, boxes, size_reduction=1, generate_method=None, join_method=join_via_max, tanh=False):
    """datautils.py:65-85 on the GPU -> (h // size_reduction, w // size_reduction) float32 on the device, one launch.

    boxes: (B,4) INTEGER xyxy (as SKU110KDataset reads them), on the host or the device; float boxes raise TypeError.  A box with
    zero reduced extent or nothing left after clipping contributes nothing (the reference raises there for two of its three
    methods: DESIGN.md 4c)."""
    from . import device_gaussians          # (kernel calls: the readers below stay host-only)
    return device_gaussians.render_full(w, h, boxes, size_reduction, generate_method, join_method, tanh)


# ---------------------------------------------------------------------------------------------------------------------
# Dataset readers of the eval commands.  Host-side, CPU: csv / json / os / PIL like the reference.
# Only what inference needs: index building + image loading; the training-time augmentations (gaussian target maps,
# flips, random crops, alpha masks) are not rebuilt and raise if asked for.
# `to_tensor` / `resize` / `pad` are torchvision 0.9 functions in the reference (PARITY UNPINNED); restated:
#   to_tensor: uint8 HWC -> float32 CHW / 255;  resize: PIL bilinear to (h, w);  pad: constant fill right / bottom.
# ---------------------------------------------------------------------------------------------------------------------
import csv as _csv
import json as _json
import os as _os
import re as _re


def pil_to_tensor(img):
    """torchvision.transforms.functional.to_tensor for 8-bit PIL images: (C,H,W) float32 in [0,1]."""
    import numpy as np
    if img.mode not in ('L', 'RGB', 'RGBA'):
        img = img.convert('RGB')
    a = np.asarray(img, dtype=np.uint8)
    if a.ndim == 2:
        a = a[:, :, None]
    return torch.from_numpy(a.copy()).permute(2, 0, 1).to(torch.float32) / 255.0


def pil_to_uint8(img):
    """The same pixels as `pil_to_tensor` as the decoder produces them: contiguous uint8 (H,W,C), no float copy.  It stands for
    the float image `u.permute(2,0,1).to(float32) / 255.0`; the product path converts it on the device (ops.device_image)."""
    import numpy as np
    if img.mode not in ('L', 'RGB', 'RGBA'):
        img = img.convert('RGB')
    a = np.asarray(img, dtype=np.uint8)
    if a.ndim == 2:
        a = a[:, :, None]
    return torch.from_numpy(a.copy()).contiguous()


IMAGE_FORMATS = ('float', 'uint8')


def _image_reader(image_format):
    """The file -> tensor step of the shelf readers: 'float' = pil_to_tensor (3,H,W) float32, 'uint8' = (H,W,3) uint8."""
    if image_format not in IMAGE_FORMATS:
        raise ValueError(f'image_format must be one of {IMAGE_FORMATS}, got {image_format!r}')
    if image_format == 'float':
        return pil_to_tensor

    def read(img):
        if img.mode != 'RGB':            # a shelf image is three planes in the 8-bit form (grey / alpha files: as RGB)
            img = img.convert('RGB')
        return pil_to_uint8(img)
    return read


def _open_image(path):
    from PIL import Image
    return Image.open(path)


class SKU110KDataset:
    """datautils.py:130-189, evaluation use (cli/gln.py:264): 8-column CSV `name,x1,y1,x2,y2,class,width,height`, one
    row per box, images grouped in order of first appearance.  Items: (image (3,H,W) float, entry dict); with
    image_format='uint8' (every shelf reader takes it) the image is (H,W,3) uint8, everything else the same."""

    def __init__(self, img_dir_path, annotation_file_path, skip=(), include_gaussians=False, flip_chance=0, image_format='float',
                 **_unused):
        if include_gaussians or flip_chance:
            raise NotImplementedError('training-time targets / augmentation are out of scope (DESIGN.md 6)')
        self.img_dir = img_dir_path
        self.read_image = _image_reader(image_format)
        self.index = self.build_index(annotation_file_path, skip)

    @staticmethod
    def build_index(annotation_file_path, skip=()):
        per_image = {}
        with open(annotation_file_path, 'r') as f:
            for row in _csv.reader(f):
                if len(row) != 8:
                    print(f'Malformed annotation row: {row}, skipping')
                    continue
                name, x1, y1, x2, y2, _, width, height = row
                if name in skip:
                    continue
                entry = per_image.setdefault(name, {'image_name': name, 'image_width': int(width), 'image_height': int(height), 'boxes': []})
                entry['boxes'].append([int(x1), int(y1), int(x2), int(y2)])
        index = list(per_image.values())
        for entry in index:
            entry['labels'] = torch.zeros(len(entry['boxes']), dtype=torch.long)
            entry['boxes'] = torch.tensor(entry['boxes'])
        return index

    def index_for_name(self, name):
        return next((i for i, e in enumerate(self.index) if e['image_name'] == name), None)

    def __len__(self):
        return len(self.index)

    def __getitem__(self, i):
        entry = dict(self.index[i])
        try:
            return self.read_image(_open_image(_os.path.join(self.img_dir, entry['image_name']))), entry
        except OSError:
            print(f'WARNING: Malformed image: {entry["image_name"]} - returning image 0 ({self.index[0]["image_name"]}) instead.')
            return self[0]


class GPBaselineDataset:
    """datautils.py:191-232: one 6-column CSV with a header row, image files under <root>/storeN/images/."""

    def __init__(self, img_dir_path, annotation_file_path, image_format='float'):
        self.read_image = _image_reader(image_format)
        self.index = self.build_index(img_dir_path, annotation_file_path)

    @staticmethod
    def build_index(image_dir_path, annotation_file_path):
        name_re = _re.compile(r'^(store\d)\_\d+.jpg$')
        per_image = {}
        with open(annotation_file_path, 'r') as f:
            for i, row in enumerate(_csv.reader(f)):
                if i == 0:
                    continue
                if len(row) != 6:
                    print(f'Malformed annotation row: {row}, skipping')
                    continue
                name, x1, y1, x2, y2, _ = row
                if name not in per_image:
                    m = name_re.match(name)
                    if m is None:
                        print(f'Malformed annotation row: {row}, skipping')
                        continue
                    per_image[name] = {'image_path': _os.path.join(image_dir_path, m.group(1), 'images', name), 'boxes': []}
                per_image[name]['boxes'].append([int(x1), int(y1), int(x2), int(y2)])
        index = list(per_image.values())
        for entry in index:
            entry['labels'] = torch.zeros(len(entry['boxes']), dtype=torch.long)
            entry['boxes'] = torch.tensor(entry['boxes'])
        return index

    def __len__(self):
        return len(self.index)

    def __getitem__(self, i):
        entry = self.index[i]
        return self.read_image(_open_image(entry['image_path'])), entry


class GroceryProductsTestSet:
    """datautils.py:623-688: GP-180, one 5-column CSV `Category/.../name.jpg, x1, y1, x2, y2` per test image, named
    s<store>_<image>.csv.  `only` / `skip` are lists of file names, or ints = keep the first `only` / drop the first
    `skip` annotations of every image (the reference's validation split).  Files are visited in sorted order (the
    reference takes os.scandir order, which is unspecified) and the label ids of `retinanet_annotations` are the sorted
    annotation strings (the reference enumerates a set)."""

    def __init__(self, image_dir, ann_dir, only=None, skip=None, retinanet_annotations=False, image_format='float'):
        self.image_dir = image_dir
        self.read_image = _image_reader(image_format)
        self.toskip = skip if type(skip) == int else 0
        self.tokeep = only if type(only) == int else 9999
        self.index = self.build_index(ann_dir, None if type(only) == int else only, None if type(skip) == int else skip)
        self.int_to_ann = sorted({ann for e in self.index for ann in e['anns']})
        self.ann_to_int = {ann: i for i, ann in enumerate(self.int_to_ann)}
        self.retinanet_annotations = retinanet_annotations

    def get_image_path(self, store, image):
        return _os.path.join(self.image_dir, f'store{store}', 'images', f'store{store}_{image}.jpg')

    def build_index(self, ann_dir, only=None, skip=None):
        file_re = _re.compile(r'^s(\d+)_(\d+)\.csv$')
        ann_re = _re.compile(r'^(.+)\.jpg')
        index = []
        for name in sorted(_os.listdir(ann_dir)):
            full = _os.path.join(ann_dir, name)
            if not _os.path.isfile(full) or (only is not None and name not in only) or (skip is not None and name in skip):
                continue
            m = file_re.match(name)
            if m is None:
                continue
            anns, boxes = [], []
            with open(full, 'r') as f:
                for row in _csv.reader(f, skipinitialspace=True):
                    if len(row) != 5:
                        print(f'Malformed annotation row in file {name}: {row}; skipping')
                        continue
                    ann, x1, y1, x2, y2 = row
                    am = ann_re.match(ann)
                    if am is None:      # (the reference prints and then fails on the next line; skipping is the stated intent)
                        print(f'Non-conforming annotation in file {name}: {ann}; skipping')
                        continue
                    anns.append(am.group(1))
                    boxes.append([int(x1), int(y1), int(x2), int(y2)])
            index.append({'id': (m.group(1), m.group(2)), 'path': self.get_image_path(m.group(1), m.group(2)),
                          'anns': anns, 'boxes': torch.tensor(boxes)})
        return index

    def get_index_for(self, store, image):
        target = self.get_image_path(store, image)
        return next((i for i, e in enumerate(self.index) if e['path'] == target), None)

    def __len__(self):
        return len(self.index)

    def __getitem__(self, i):
        e = self.index[i]
        img = self.read_image(_open_image(e['path']))
        anns, boxes = e['anns'][self.toskip:self.tokeep], e['boxes'][self.toskip:self.tokeep]
        if self.retinanet_annotations:
            return img, {'labels': torch.tensor([self.ann_to_int[a] for a in anns], dtype=torch.long), 'boxes': boxes}
        return img, anns, boxes


class PlanogramTestSet(GroceryProductsTestSet):
    """datautils.py:692-707: GP-180 test images + their Tonioni planograms (s<store>_<image>.json)."""

    def __init__(self, image_dir, ann_dir, plano_dir, only=None, skip=None, image_format='float'):
        self.plano_dir = plano_dir
        super().__init__(image_dir, ann_dir, only, skip, image_format=image_format)

    def build_index(self, ann_dir, only=None, skip=None):
        from . import planogram_adapters
        index = super().build_index(ann_dir, only, skip)
        for e in index:
            s, i = e['id']
            boxes, labels, g = planogram_adapters.read_tonioni_planogram(_os.path.join(self.plano_dir, f's{s}_{i}.json'))
            e['plano'] = {'boxes': boxes, 'labels': labels, 'graph': g, 'actual_accuracy': 1.0}
        return index

    def __getitem__(self, i):
        img, anns, boxes = super().__getitem__(i)
        return img, anns, boxes, self.index[i]['plano']


class InternalPlanoSet:
    """datautils.py:709-750: index.json -> [{image, planogram, correct, facings}], planogram = [{code, box}] with the
    y axis pointing up (flipped here to detector coordinates)."""

    def __init__(self, dir, image_format='float'):
        self.read_image = _image_reader(image_format)
        self.index = self.build_index(dir)

    @staticmethod
    def build_index(dir):
        with open(_os.path.join(dir, 'index.json'), 'r') as f:
            listing = _json.load(f)
        res = []
        for obj in listing:
            with open(_os.path.join(dir, obj['planogram']), 'r') as f:
                plano = _json.load(f)
            boxes = torch.tensor([e['box'] for e in plano], dtype=torch.float)
            top = boxes[:, 3].max()
            y1, y2 = top - boxes[:, 3], top - boxes[:, 1]
            boxes[:, 1], boxes[:, 3] = y1, y2
            res.append({'img': _os.path.join(dir, obj['image']), 'anns': [e['code'] for e in plano], 'boxes': boxes,
                        'actual_accuracy': obj['correct'] / obj['facings']})
        return res

    def __len__(self):
        return len(self.index)

    def __getitem__(self, i):
        e = self.index[i]
        return self.read_image(_open_image(e['img'])), {'labels': e['anns'], 'boxes': e['boxes'], 'actual_accuracy': e['actual_accuracy']}


class GroceryProductsDataset:
    """datautils.py:301-451, gallery use (`include_annotations=True`, cli/eval.py:45): walks the GP training tree
    (<root>/<category>/.../<name>.<ext>), skipping hierarchies that match `skip`; annotation = 'Category/.../name'.
    Items: (image, image, categories[, annotation]) with the image resized so that its longer side is 256, scaled to
    [-1,1] and padded right / bottom with 0 to 256x256 (`tensorize`, :397-415).  Directory entries are visited in sorted
    order (the reference takes os.scandir order).  Random crops and masks are training-time and not rebuilt.
    image_format='uint8': the image of an item is the resized (h,w,3) uint8 image itself -- a gallery byte image, which
    stands for the float item `gallery_float` makes of it; nothing after PIL's resize runs on the host."""

    IGNORED_FILES = ('.DS_Store', 'index.txt', 'TrainingClassesIndex.mat', 'classes.csv', 'Thumbs.db')

    def __init__(self, image_roots, skip=(r'^Background.*$', r'^.*/[Oo]riginals?$'), only=None, random_crop=False,
                 resize=True, test_can_load=False, include_annotations=False, include_masks=False, index_from_file=False,
                 image_format='float', **_unused):
        if include_masks:
            raise NotImplementedError('training-time masks are out of scope (DESIGN.md 6)')
        if image_format not in IMAGE_FORMATS:
            raise ValueError(f'image_format must be one of {IMAGE_FORMATS}, got {image_format!r}')
        if image_format == 'uint8' and not resize:
            raise ValueError("image_format='uint8' needs resize=True: a gallery byte image is at most 256 x 256 (unresized items cannot be batched in either form)")
        self.image_format = image_format
        if isinstance(image_roots, str):
            image_roots = (image_roots,)
        skip_re = _re.compile('|'.join(f'({s})' for s in skip))
        build = self.build_index_from_file if index_from_file else self.build_index
        self.paths, self.categories, self.annotations = build(image_roots, skip_re, only, test_can_load)
        self.resize = resize
        self.include_annotations = include_annotations

    @classmethod
    def build_index(cls, image_roots, skip, only=None, test_can_load=False):
        stem_re = _re.compile(r'^(.+)\.\w+$')
        paths, categories, annotations = [], [], []
        for root in image_roots:
            stack = [(root, [])]
            while stack:
                cur, hier = stack.pop()
                if skip.match('/'.join(hier)) is not None:
                    continue
                if only is not None and hier and hier[0] not in only:
                    continue
                for name in sorted(_os.listdir(cur)):
                    full = _os.path.join(cur, name)
                    if _os.path.isdir(full) and not _os.path.islink(full):
                        stack.append((full, hier + [name]))
                    elif _os.path.isfile(full):
                        if name in cls.IGNORED_FILES or skip.match('/'.join(hier + [name])):
                            continue
                        if test_can_load:
                            try:
                                _open_image(full)
                            except OSError:
                                continue
                        m = stem_re.match(name)
                        if m is None:
                            print(f'Nonconforming filename: {name}, skipping')
                            continue
                        paths.append(full)
                        categories.append(hier)
                        annotations.append('/'.join(hier + [m.group(1)]))
        return paths, categories, annotations

    @staticmethod
    def build_index_from_file(dataset_roots, skip, only=None, test_can_load=False, index_filename='TrainingFiles.txt'):
        paths, categories, annotations = [], [], []
        for root in dataset_roots:
            with open(_os.path.join(root, index_filename), 'r') as f:
                for line in f:
                    parts = line.strip().split('/')
                    if len(parts) < 2:
                        continue
                    hier = parts[1:-1]          # drop the leading "Training" folder and the file name
                    if only is not None and hier[0] not in only:
                        continue
                    if skip.match('/'.join(hier)) is not None:
                        continue
                    paths.append(_os.path.join(root, *parts))
                    categories.append(hier)
                    annotations.append('/'.join(parts[1:]))
        return paths, categories, annotations

    def index_for_ann(self, ann):
        return next((i for i, a in enumerate(self.annotations) if a == ann), None)

    @staticmethod
    def _resized(img):
        """The PIL image resized so that its longer side is 256 (the step both item forms share)."""
        from PIL import Image
        S = CLASSIFICATION_IMAGE_SIZE
        h, w = (S, round(S * img.width / img.height)) if img.height > img.width else (round(S * img.height / img.width), S)
        return img.resize((w, h), Image.BILINEAR), h, w

    def byteize(self, img):
        """The uint8 item of an RGB PIL image: the resized image's own bytes, (h,w,3)."""
        return pil_to_uint8(self._resized(img)[0])[:, :, :3].contiguous()

    def _item(self, img, i):
        t = self.byteize(img) if self.image_format == 'uint8' else self.tensorize(img, True)
        if self.include_annotations:
            return t, t, self.categories[i], self.annotations[i]
        return t, t, self.categories[i]

    def tensorize(self, img, tanh=False):
        if not self.resize:
            return pil_to_tensor(img)
        S = CLASSIFICATION_IMAGE_SIZE
        img, h, w = self._resized(img)
        t = pil_to_tensor(img)[:3]
        if tanh:
            t = t * 2 - 1
        out = torch.full((t.shape[0], S, S), 0.0 if tanh else 0.5)
        out[:, :h, :w] = t
        return out

    def __len__(self):
        return len(self.paths)

    def __getitem__(self, i):
        img = _open_image(self.paths[i])
        if img.mode != 'RGB':
            img = img.convert('RGB')
        return self._item(img, i)


def gallery_float(u8, size=CLASSIFICATION_IMAGE_SIZE):
    """The float image a gallery byte image stands for: (h,w,3) uint8, 1 <= h, w <= size -> (3,size,size) float32, the
    content `uint8_table[b] * 2 - 1` (torch float32 arithmetic on the host, the very values `tensorize(img, tanh=True)` computes),
    everything at y >= h or x >= w 0.0.  The host definition: tests, documents and the GALLERY_U8-off route of `Classifier.build_index`
    use it, the product path's kernel looks the same values up in a table."""
    from .ops import uint8_table
    if not (torch.is_tensor(u8) and u8.dtype == torch.uint8 and u8.dim() == 3 and u8.shape[2] == 3):
        raise TypeError(f'a gallery byte image is a (h,w,3) uint8 tensor, got {type(u8).__name__} {tuple(getattr(u8, "shape", ()))}')
    h, w = int(u8.shape[0]), int(u8.shape[1])
    if not (1 <= h <= size and 1 <= w <= size):
        raise ValueError(f'a gallery byte image is at most {size} x {size} and not empty, got {h} x {w}')
    idx = u8.cpu().permute(2, 0, 1).to(torch.int64)
    out = torch.full((3, size, size), 0.0)
    out[:, :h, :w] = uint8_table()[idx] * 2 - 1
    return out


class InternalTrainSet(GroceryProductsDataset):
    """datautils.py:453-482: product renders with an alpha channel; the annotation is the numeric product code at the
    end of the path, transparent pixels become white."""

    def __init__(self, root, skip=(r'^Unknown.*$',), resize=True, include_annotations=False, image_format='float', **_unused):
        super().__init__([root], skip=skip, resize=resize, include_annotations=include_annotations, image_format=image_format)
        code_re = _re.compile(r'^(.+/)*(\d+)')
        self.annotations = [code_re.match(a).group(2) for a in self.annotations]

    def index_for_ann(self, ann):
        best = None
        for i, a in enumerate(self.annotations):
            if a != ann:
                continue
            if 'front' in self.categories[i]:
                return i
            if 'back' in self.categories[i] or best is None:
                best = i if ('back' in self.categories[i] or best is None) else best
        return best

    def __getitem__(self, i):
        from PIL import Image
        img = _open_image(self.paths[i]).convert('RGBA')
        if self.image_format == 'uint8':
            # transparent -> white on the bytes: the float code below goes through the same bytes ((b / 255 * 255).round() == b)
            a = pil_to_uint8(img).numpy()
            rgb = a[:, :, :3].copy()
            rgb[a[:, :, 3] == 0] = 255
            return self._item(Image.fromarray(rgb, 'RGB'), i)
        white = Image.new('RGBA', img.size, (255, 255, 255, 255))
        a = pil_to_tensor(img)
        rgb = a[:3].clone()
        rgb[:, a[3] == 0] = 1.0
        img = Image.fromarray((rgb.permute(1, 2, 0) * 255).round().to(torch.uint8).numpy(), 'RGB')
        del white
        t = self.tensorize(img, True)
        if self.include_annotations:
            return t, t, self.categories[i], self.annotations[i]
        return t, t, self.categories[i]


class SimpleFolderSet:
    """datautils.py:484-512, the bring-your-own-data gallery of `misc pipeline-demo`: a folder of product photos named after their
    label -- `<label>.png`, `.jpg` or `.jpeg` (`types`; the label is the file name without that ending, whatever else it holds).
    Items: (img, img, label, label), doubled as the other sets' are; transparent pixels (alpha 0) become white and the alpha plane is
    dropped.  train=False: the image as it is, float (3, h, w) in [0, 1] of any size -- what the scene is rebuilt from
    (`rendering.ThumbnailAtlas(..., float_items='unit')`).  train=True: `resize_for_classification` of it, (3, 256, 256) in [0, 1] on
    `device` (the kernel has no host form) -- what the reference embeds as its gallery, although the encoder's queries are in [-1, 1]
    (SURVEY.md Appendix B); scale=True applies `scale_to_tanh` (x * 2 - 1) to such an item, the range the encoder was trained on.
    Directory entries are visited in sorted order, as this module's other sets visit them (the reference takes os.scandir order)."""

    def __init__(self, root, train=True, types=('.png', '.jpg', '.jpeg'), device='cuda', scale=False):
        self.paths, self.classes = self.build_index(root, types)
        self.train, self.device, self.scale = train, device, scale

    @staticmethod
    def build_index(root, types):
        name_re = _re.compile('^(.*)(' + '|'.join(_re.escape(t) for t in types) + ')$')
        paths, classes = [], []
        for name in sorted(_os.listdir(root)):
            m = name_re.match(name)
            if m is None or not _os.path.isfile(_os.path.join(root, name)):
                continue
            paths.append(_os.path.join(root, name))
            classes.append(m.group(1))
        return paths, classes

    def index_for_ann(self, ann):
        return self.classes.index(ann)

    def __len__(self):
        return len(self.paths)

    def __getitem__(self, i):
        c = self.classes[i]
        img = pil_to_tensor(_open_image(self.paths[i]))
        if len(img) > 3:
            img[:, img[3] == 0] = 1
            img = img[:3]                       # drop alpha
        elif len(img) == 1:
            img = img.expand(3, -1, -1).contiguous()
        if self.train:
            img = resize_for_classification(img.to(self.device))
            if self.scale:
                img = img * 2 - 1
        return img, img, c, c


def read_planogram_json(path):
    """The planogram file of `misc pipeline-demo` (cli/misc.py:127-139, 171-174): a JSON list of {"label": ..., "box": [x1, y1, x2, y2]}
    -> {'boxes': float32 (n, 4), 'labels': list of n} as the comparator takes it."""
    with open(path) as f:
        plano = _json.load(f)
    if not isinstance(plano, list) or not all(isinstance(o, dict) and 'label' in o and 'box' in o and len(o['box']) == 4 for o in plano):
        raise ValueError(f'{path}: a planogram is a JSON list of {{"label": ..., "box": [x1, y1, x2, y2]}}')
    return {'boxes': torch.tensor([o['box'] for o in plano], dtype=torch.float32).reshape(-1, 4), 'labels': [o['label'] for o in plano]}
