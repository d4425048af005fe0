"""`cvpce` command line, evaluation surface only (reference: cvpce/cli/__init__.py, cli/gln.py:230-307,
cli/dihe.py:257-309,382-423, cli/eval.py:12-71,168-240): the same command names, arguments, options and defaults as the
reference for

    cvpce gln eval | gln detect | gln seek-sku110k-outliers | dihe eval | dihe prebuild-index | eval-product-detection |
    eval-planograms | rebuild-scene | plot-planogram-eval | misc pipeline-demo

(the last two write the step pictures of `rendering.StepPictures` to --out PREFIX instead of opening matplotlib windows; the demo's
embedding scatter plots are not drawn, and `misc pipeline-demo --scale-gallery` goes beyond the reference, see its help text).
Training, hyper-parameter search, dataset visualisation and the other plotting commands are out of scope (`gln seek-sku110k-outliers` scores
the three training losses forward only, in eval mode, and adds --batch-size and --dataloader-workers: cli/gln.py:309-377).  Options that only steer
the reference's matplotlib (`--plots`, `--plot-res-reduction`) are accepted and ignored: every metric is printed.
`--dataloader-workers` is the number of reader THREADS of `feeding.ImageFeeder`: the shelf images are opened in the 8-bit
form, decoded that many at a time ahead of the kernels and uploaded from pinned memory (0 = read serially in the calling
thread; the printed metrics are the same to the last digit, the inputs being the same bits).  The two whole-pipeline commands
have no such option in the reference: they read the same way, with CVPCE_DATALOADER_WORKERS threads (default 8).
One switch goes beyond the reference: `gln eval` and `eval-product-detection` take --device-metrics / --no-device-metrics
(default off: the matching behind mAP runs on the GPU instead of on the host; `_DeviceMetricsCommand`), `gln eval` also
--gaussian-loss / --no-gaussian-loss with --gaussian-outlier-threshold (default off: every image's Gaussian map is scored on the GPU
against the map rendered from its ground-truth boxes, the reference's gaussian_loss; `_GaussianLossCommand`), `eval-planograms` takes
--device-graphs, --device-tail, --device-reclass and --device-detections (default off; `_DeviceDetectionsCommand`) and --report FILE
(one JSON line per image saying which positions are missing and what is there; `_ReportCommand`) and --render DIR (the three compliance
pictures of every image as PNG files; `_RenderCommand`) and --matcher [large|tonioni] (default large: the comparator's graph matcher;
`_MatcherCommand`), `rebuild-scene` writes those pictures for one image (--out PREFIX instead of the
reference's matplotlib window), and `dihe eval` takes --device-eval /
--no-device-eval (default off: EVAL_WINDOW images at a time are cropped, embedded and matched in one pass and compared on the GPU;
`_DeviceEvalCommand`).

    python -m cvpce_amd.cli --help
"""
import json
import os

import click
import torch

from .. import classification_eval, datautils, detection_eval, feeding, production, proposals_eval
from ..defaults import (GP_ANN_DIR, GP_PLANO_DIR, GP_TEST_DIR, GP_TEST_VALIDATION_SET_SIZE, GP_TRAIN_FOLDERS, OUT_DIR,
                        SKU110K_ANNOTATION_FILE, SKU110K_IMG_DIR, SKU110K_SKIP)
from ..models import classification, proposals

MODEL_STATE_DICT_KEY = 'model_state_dict'          # proposals_training.py / classification_training.py checkpoint keys
EMBEDDER_STATE_DICT_KEY = 'model_state_dict'

_DIR = dict(exists=True, file_okay=False, dir_okay=True, readable=True)
_FILE = dict(exists=True, file_okay=True, dir_okay=False, readable=True)


EVAL_WINDOW = 8     # images read ahead and run through the kernels together by the evaluation commands


def _reader_threads():
    """Reader threads of the two whole-pipeline commands.  The reference gives them no --dataloader-workers option (it hard-codes its
    loaders there) and the option set of every command is the reference's, so the count comes from the environment:
    CVPCE_DATALOADER_WORKERS, default 8 (the reference's DataLoader default), 0 = read serially in the calling thread."""
    return max(0, int(os.environ.get('CVPCE_DATALOADER_WORKERS', feeding.DEFAULT_WORKERS)))


def _coco_or(thresholds, coco):
    return [f.item() for f in torch.linspace(.5, .95, 10)] if coco else list(thresholds)


def _load_encoder(dihe_state):
    encoder = classification.macvgg_embedder(model='vgg16', pretrained=False).cuda()
    state = torch.load(dihe_state, map_location='cpu')
    encoder.load_state_dict(state[EMBEDDER_STATE_DICT_KEY])
    return encoder.eval().requires_grad_(False)


class _DeviceMetricsCommand(click.Command):
    """A command that also takes --device-metrics / --no-device-metrics (default: off).

    The declared options of every command are the reference's, name by name and default by default; this switch has no
    counterpart there.  It is therefore not declared among them: it is taken off the argument list before click parses the
    rest, shown in --help under a heading of its own, and read by the command through `_device_metrics_switch()`."""
    SWITCH = {'--device-metrics': True, '--no-device-metrics': False}
    HELP = ('Match detections to the ground truth on the GPU instead of on the host (cvpce_amd.device_metrics). '
            'No metric process is started: --metric-workers is ignored with it.  [default: off]')

    KEY = 'cvpce_amd.device_metrics'
    LABEL = '--device-metrics / --no-device-metrics'

    def parse_args(self, ctx, args):
        rest = []
        ctx.meta[self.KEY] = False
        for i, a in enumerate(args):
            if a == '--':                        # (everything after it is positional)
                rest += args[i:]
                break
            if a in self.SWITCH:
                ctx.meta[self.KEY] = self.SWITCH[a]
            else:
                rest.append(a)
        return super().parse_args(ctx, rest)

    def format_options(self, ctx, formatter):
        super().format_options(ctx, formatter)
        with formatter.section('Options beyond the reference\'s'):
            formatter.write_dl([(self.LABEL, self.HELP)] + list(self.MORE))

    MORE = ()                                    # further (label, help) rows of a subclass with a second switch


def _device_metrics_switch():
    return bool(click.get_current_context().meta.get('cvpce_amd.device_metrics', False))


class _DeviceGraphsCommand(_DeviceMetricsCommand):
    """The same arrangement for --device-graphs / --no-device-graphs (default: off) of the planogram command."""
    SWITCH = {'--device-graphs': True, '--no-device-graphs': False}
    HELP = ('Build the neighbour graphs and match them on the GPU instead of on the host (cvpce_amd.planograms_device; its order at '
            'equal distances is the documented device rule).  [default: off]')
    KEY = 'cvpce_amd.device_graphs'
    LABEL = '--device-graphs / --no-device-graphs'


def _device_graphs_switch():
    return bool(click.get_current_context().meta.get(_DeviceGraphsCommand.KEY, False))


class _DeviceTailCommand(_DeviceGraphsCommand):
    """--device-graphs as above, and --device-tail / --no-device-tail (default: off) beside it, arranged the same way."""
    TAIL_SWITCH = {'--device-tail': True, '--no-device-tail': False}
    TAIL_HELP = ('Also run the homography, the projection and the per-label claim on the GPU (cvpce_amd.planograms_device.finalize_batch; '
                 'the documented tail rule).  Needs --device-graphs: without it the command stops with an error.  [default: off]')
    TAIL_KEY = 'cvpce_amd.device_tail'
    TAIL_LABEL = '--device-tail / --no-device-tail'

    def parse_args(self, ctx, args):
        rest = []
        ctx.meta[self.TAIL_KEY] = False
        for i, a in enumerate(args):
            if a == '--':
                rest += args[i:]
                break
            if a in self.TAIL_SWITCH:
                ctx.meta[self.TAIL_KEY] = self.TAIL_SWITCH[a]
            else:
                rest.append(a)
        graphs = [self.SWITCH[a] for a in (rest[:rest.index('--')] if '--' in rest else rest) if a in self.SWITCH]
        if ctx.meta[self.TAIL_KEY] and not (graphs and graphs[-1]) and not ctx.resilient_parsing:
            raise click.UsageError('--device-tail needs --device-graphs', ctx)          # (it implies nothing on its own)
        return super().parse_args(ctx, rest)

    MORE = ((TAIL_LABEL, TAIL_HELP),)


def _device_tail_switch():
    return bool(click.get_current_context().meta.get(_DeviceTailCommand.TAIL_KEY, False))


class _DeviceReclassCommand(_DeviceTailCommand):
    """The two switches above, and --device-reclass / --no-device-reclass (default: off) beside them, arranged the same way."""
    RECLASS_SWITCH = {'--device-reclass': True, '--no-device-reclass': False}
    RECLASS_HELP = ('Also re-classify a window\'s expected-but-undetected positions in one GPU pass instead of image by image through the '
                    'host (cvpce_amd.planograms_device.reclassify_batch; the documented re-classification rule).  Needs --device-tail: '
                    'without it the command stops with an error.  [default: off]')
    RECLASS_KEY = 'cvpce_amd.device_reclass'
    RECLASS_LABEL = '--device-reclass / --no-device-reclass'

    def parse_args(self, ctx, args):
        rest = []
        ctx.meta[self.RECLASS_KEY] = False
        for i, a in enumerate(args):
            if a == '--':
                rest += args[i:]
                break
            if a in self.RECLASS_SWITCH:
                ctx.meta[self.RECLASS_KEY] = self.RECLASS_SWITCH[a]
            else:
                rest.append(a)
        tails = [self.TAIL_SWITCH[a] for a in (rest[:rest.index('--')] if '--' in rest else rest) if a in self.TAIL_SWITCH]
        if ctx.meta[self.RECLASS_KEY] and not (tails and tails[-1]) and not ctx.resilient_parsing:
            raise click.UsageError('--device-reclass needs --device-tail', ctx)        # (it implies nothing on its own)
        return super().parse_args(ctx, rest)

    MORE = _DeviceTailCommand.MORE + ((RECLASS_LABEL, RECLASS_HELP),)


def _device_reclass_switch():
    return bool(click.get_current_context().meta.get(_DeviceReclassCommand.RECLASS_KEY, False))


class _DeviceDetectionsCommand(_DeviceReclassCommand):
    """The three switches above, and --device-detections / --no-device-detections (default: off) beside them, arranged the same way."""
    DETECTIONS_SWITCH = {'--device-detections': True, '--no-device-detections': False}
    DETECTIONS_HELP = ('Also keep a window\'s detections on the GPU from the matcher to the comparator instead of copying them to the host '
                       '(cvpce_amd.planograms_device.DeviceActuals; the documented detections rule).  Needs --device-tail: without it the '
                       'command stops with an error.  [default: off]')
    DETECTIONS_KEY = 'cvpce_amd.device_detections'
    DETECTIONS_LABEL = '--device-detections / --no-device-detections'

    def parse_args(self, ctx, args):
        rest = []
        ctx.meta[self.DETECTIONS_KEY] = False
        for i, a in enumerate(args):
            if a == '--':
                rest += args[i:]
                break
            if a in self.DETECTIONS_SWITCH:
                ctx.meta[self.DETECTIONS_KEY] = self.DETECTIONS_SWITCH[a]
            else:
                rest.append(a)
        tails = [self.TAIL_SWITCH[a] for a in (rest[:rest.index('--')] if '--' in rest else rest) if a in self.TAIL_SWITCH]
        if ctx.meta[self.DETECTIONS_KEY] and not (tails and tails[-1]) and not ctx.resilient_parsing:
            raise click.UsageError('--device-detections needs --device-tail', ctx)        # (it implies nothing on its own)
        return super().parse_args(ctx, rest)

    MORE = _DeviceReclassCommand.MORE + ((DETECTIONS_LABEL, DETECTIONS_HELP),)


def _device_detections_switch():
    return bool(click.get_current_context().meta.get(_DeviceDetectionsCommand.DETECTIONS_KEY, False))


class _ReportCommand(_DeviceDetectionsCommand):
    """The four switches above, and --report FILE (default: none) beside them, arranged the same way."""
    REPORT_OPTION = '--report'
    REPORT_HELP = ('Also write one JSON line per image to FILE: which expected positions were detected, recovered, missing, out of view or '
                   'unchecked, what sits there instead and which detections the planogram does not know '
                   '(cvpce_amd.production.ComplianceReport.to_dict, plus the image index).  [default: none]')
    REPORT_KEY = 'cvpce_amd.report'
    REPORT_LABEL = '--report FILE'

    def parse_args(self, ctx, args):
        rest, args = [], list(args)
        ctx.meta[self.REPORT_KEY] = None
        i = 0
        while i < len(args):
            a = args[i]
            if a == '--':
                rest += args[i:]
                break
            if a == self.REPORT_OPTION:
                if i + 1 >= len(args):
                    raise click.UsageError('--report needs a file name', ctx)
                ctx.meta[self.REPORT_KEY] = args[i + 1]
                i += 1
            elif a.startswith(self.REPORT_OPTION + '='):
                ctx.meta[self.REPORT_KEY] = a[len(self.REPORT_OPTION) + 1:]
            else:
                rest.append(a)
            i += 1
        return super().parse_args(ctx, rest)

    MORE = _DeviceDetectionsCommand.MORE + ((REPORT_LABEL, REPORT_HELP),)


def _report_file():
    return click.get_current_context().meta.get(_ReportCommand.REPORT_KEY)


class _RenderCommand(_ReportCommand):
    """The switches and --report above, and --render DIR (default: none) beside them, arranged the same way."""
    RENDER_OPTION = '--render'
    RENDER_HELP = ('Also write the three compliance pictures of every image to DIR as <index>_annotated.png, <index>_observed.png and '
                   '<index>_expected.png (cvpce_amd.rendering.CompliancePictures: composed on the GPU, encoded on the host).  [default: none]')
    RENDER_KEY = 'cvpce_amd.render'
    RENDER_LABEL = '--render DIR'

    def parse_args(self, ctx, args):
        rest, args = [], list(args)
        ctx.meta[self.RENDER_KEY] = None
        i = 0
        while i < len(args):
            a = args[i]
            if a == '--':
                rest += args[i:]
                break
            if a == self.RENDER_OPTION:
                if i + 1 >= len(args):
                    raise click.UsageError('--render needs a directory', ctx)
                ctx.meta[self.RENDER_KEY] = args[i + 1]
                i += 1
            elif a.startswith(self.RENDER_OPTION + '='):
                ctx.meta[self.RENDER_KEY] = a[len(self.RENDER_OPTION) + 1:]
            else:
                rest.append(a)
            i += 1
        return super().parse_args(ctx, rest)

    MORE = _ReportCommand.MORE + ((RENDER_LABEL, RENDER_HELP),)


def _render_dir():
    return click.get_current_context().meta.get(_RenderCommand.RENDER_KEY)


class _MatcherCommand(_RenderCommand):
    """The switches, --report and --render above, and --matcher [large|tonioni] (default: large) beside them, arranged the same way."""
    MATCHER_OPTION = '--matcher'
    MATCHERS = production.PlanogramComparator.MATCHERS
    MATCHER_HELP = ('The graph matcher of the comparator: large, the first sufficiently large common subgraph, or tonioni, the largest of '
                    'the greedy runs from every hypothesis on (cvpce_amd.planograms.tonioni_mcs; with --device-graphs it runs on the GPU, the '
                    'documented Tonioni rule): a larger matching on shelves with many facings of few products.  [default: large]')
    MATCHER_KEY = 'cvpce_amd.matcher'
    MATCHER_LABEL = '--matcher [large|tonioni]'

    def parse_args(self, ctx, args):
        rest, args = [], list(args)
        ctx.meta[self.MATCHER_KEY] = self.MATCHERS[0]
        i = 0
        while i < len(args):
            a = args[i]
            if a == '--':
                rest += args[i:]
                break
            if a == self.MATCHER_OPTION:
                if i + 1 >= len(args):
                    raise click.UsageError('--matcher needs a name', ctx)
                ctx.meta[self.MATCHER_KEY] = args[i + 1]
                i += 1
            elif a.startswith(self.MATCHER_OPTION + '='):
                ctx.meta[self.MATCHER_KEY] = a[len(self.MATCHER_OPTION) + 1:]
            else:
                rest.append(a)
            i += 1
        if ctx.meta[self.MATCHER_KEY] not in self.MATCHERS and not ctx.resilient_parsing:
            raise click.UsageError(f'--matcher is one of {", ".join(self.MATCHERS)}', ctx)
        return super().parse_args(ctx, rest)

    MORE = _RenderCommand.MORE + ((MATCHER_LABEL, MATCHER_HELP),)


def _matcher_name():
    return click.get_current_context().meta.get(_MatcherCommand.MATCHER_KEY, _MatcherCommand.MATCHERS[0])


class _DeviceEvalCommand(_DeviceMetricsCommand):
    """The same arrangement for --device-eval / --no-device-eval (default: off) of `dihe eval`."""
    SWITCH = {'--device-eval': True, '--no-device-eval': False}
    HELP = ('Crop, embed and match a window of test images in one GPU pass and compare label ids there instead of image by image '
            'through the host (cvpce_amd.device_classification; the same counts).  [default: off]')
    KEY = 'cvpce_amd.device_eval'
    LABEL = '--device-eval / --no-device-eval'


def _device_eval_switch():
    return bool(click.get_current_context().meta.get(_DeviceEvalCommand.KEY, False))


class _GaussianLossCommand(_DeviceMetricsCommand):
    """--device-metrics as above, and beside it --gaussian-loss / --no-gaussian-loss (default: off) with its
    --gaussian-outlier-threshold VALUE (default 3), arranged the same way: taken off the argument list before click parses the
    reference's options."""
    GAUSS_SWITCH = {'--gaussian-loss': True, '--no-gaussian-loss': False}
    GAUSS_HELP = ('Also score every image\'s Gaussian map against the map rendered from its ground-truth boxes, on the GPU behind the detector '
                  '(cvpce_amd.device_gaussians; the reference\'s gaussian_loss).  SKU-110K only: its boxes are integers.  [default: off]')
    GAUSS_KEY = 'cvpce_amd.gaussian_loss'
    GAUSS_LABEL = '--gaussian-loss / --no-gaussian-loss'
    THRESHOLD = '--gaussian-outlier-threshold'
    THRESHOLD_HELP = 'An image is an outlier when its loss exceeds mean + FLOAT * std of all losses (with --gaussian-loss).  [default: 3]'
    THRESHOLD_KEY = 'cvpce_amd.gaussian_outlier_threshold'

    def parse_args(self, ctx, args):
        rest, i = [], 0
        ctx.meta[self.GAUSS_KEY], ctx.meta[self.THRESHOLD_KEY] = False, 3.0
        while i < len(args):
            a = args[i]
            if a == '--':
                rest += args[i:]
                break
            value = None
            if a == self.THRESHOLD:
                i += 1
                value = args[i] if i < len(args) else None
                if value is None and not ctx.resilient_parsing:
                    raise click.UsageError(f'{self.THRESHOLD} needs a value', ctx)
            elif a.startswith(self.THRESHOLD + '='):
                value = a.split('=', 1)[1]
            elif a in self.GAUSS_SWITCH:
                ctx.meta[self.GAUSS_KEY] = self.GAUSS_SWITCH[a]
            else:
                rest.append(a)
            if value is not None:
                try:
                    ctx.meta[self.THRESHOLD_KEY] = float(value)
                except ValueError:
                    raise click.UsageError(f'{self.THRESHOLD}: {value!r} is not a number', ctx)
            i += 1
        return super().parse_args(ctx, rest)

    MORE = ((GAUSS_LABEL, GAUSS_HELP), (THRESHOLD + ' FLOAT', THRESHOLD_HELP))


def _gaussian_loss_switch():
    """-> the outlier threshold when --gaussian-loss is on, else None"""
    meta = click.get_current_context().meta
    return meta.get(_GaussianLossCommand.THRESHOLD_KEY, 3.0) if meta.get(_GaussianLossCommand.GAUSS_KEY, False) else None


@click.group()
def cli():
    """Computer vision based planogram compliance evaluation -- MI355X inference / evaluation commands."""


# ------------------------------------------------------------------ gln ------------------------------------------------
@cli.group()
def gln():
    """Product proposal generation (GLN)."""


@gln.command(cls=_GaussianLossCommand)
@click.option('--dataset', type=click.Choice(('sku110k', 'gp180', 'gpbaseline')), default='sku110k', show_default=True,
              help='Dataset type that --imgs and --annotations points to')
@click.option('--imgs', type=click.Path(**_DIR), default=SKU110K_IMG_DIR, show_default=True, help='Path to image dir')
@click.option('--annotations', type=click.Path(exists=True), default=SKU110K_ANNOTATION_FILE, show_default=True,
              help='Path to annotations used for testing')
@click.option('--batch-size', type=int, default=1, show_default=True, help='Batch size')
@click.option('--dataloader-workers', type=int, default=4, show_default=True, help='Number of data loading threads (0 = read in the calling thread)')
@click.option('--metric-workers', type=int, default=8, show_default=True,
              help='Number of metric calculating processes (0 = in-process); ignored with --device-metrics')
@click.option('--iou-threshold', '-t', type=float, multiple=True, default=(0.5,), show_default=True,
              help='IoU thresholds to calculate metrics for')
@click.option('--coco/--no-coco', default=False, show_default=True,
              help="Whether to use COCO IoU thresholds instead of whatever's set in --iou-threshold")
@click.option('--trim-module-prefix/--no-trim-module-prefix', default=False, show_default=True,
              help='Trim "module." prefix from loaded model')
@click.option('--plots/--no-plots', default=True, show_default=True, help='(ignored) precision-recall curves are not drawn')
@click.option('--plot-res-reduction', type=int, default=200, show_default=True, help='(ignored)')
@click.argument('state-file', type=click.Path(**_FILE))
def eval(dataset, imgs, annotations, batch_size, dataloader_workers, metric_workers, iou_threshold, coco,
         trim_module_prefix, plots, plot_res_reduction, state_file):
    """Evaluate product proposal generation performance.

    STATE_FILE should point to some GLN weights."""
    outlier_threshold = _gaussian_loss_switch()
    if outlier_threshold is not None and dataset != 'sku110k':
        raise click.UsageError('--gaussian-loss needs --dataset sku110k: Gaussian targets are rendered from integer boxes')
    gaussian_score = None
    if outlier_threshold is not None:
        from .. import device_gaussians
        gaussian_score = lambda model: device_gaussians.GaussianScore(model, outlier_threshold=outlier_threshold)  # noqa: E731
    if dataset == 'sku110k':
        data = datautils.SKU110KDataset(imgs, annotations, skip=SKU110K_SKIP, include_gaussians=False, flip_chance=0, image_format='uint8')
    elif dataset == 'gp180':
        data = datautils.GroceryProductsTestSet(imgs, annotations, retinanet_annotations=True, image_format='uint8')
    else:
        data = datautils.GPBaselineDataset(imgs, annotations, image_format='uint8')
    thresholds = _coco_or(iou_threshold, coco)
    evaluation = proposals_eval.evaluate_gln(state_file, data, thresholds=thresholds, batch_size=batch_size,
                                             num_workers=dataloader_workers, num_metric_processes=metric_workers, trim_module_prefix=trim_module_prefix,
                                             device_metrics=_device_metrics_switch(), gaussian_score=gaussian_score)
    ap = ar = 0
    for t in thresholds:
        print(f'{t}:\t{evaluation[t]}')
        ap += evaluation[t]['ap']
        ar += evaluation[t]['ar_300']
    print(f'--> AP {ap / len(thresholds)}')
    print(f'--> AR300 {ar / len(thresholds)}')
    if gaussian_score is not None:
        scored = evaluation['gaussians']
        print(f'--> Gaussian loss {scored["mean"]} (std {scored["std"]})')
        for i in scored['outliers']:
            print(f'Outlier at index {i}: {data.index[i]["image_name"]}\t{float(scored["loss"][i])}')


@gln.command(name='seek-sku110k-outliers')
@click.option('--imgs', type=click.Path(**_DIR), default=SKU110K_IMG_DIR, show_default=True, help='Path to SKU-110K image dir')
@click.option('--annotations', type=click.Path(exists=True), default=SKU110K_ANNOTATION_FILE, show_default=True,
              help='Path to SKU-110K annotation file used in iteration')
@click.option('--outlier-threshold', type=int, default=3, show_default=True,
              help='The minimum number of standard deviations a loss needs to be above the average for an image to be considered an outlier')
@click.option('--trim-module-prefix/--no-trim-module-prefix', default=False, show_default=True,
              help='Trim "module." prefix from loaded model, legacy option, shouldn\'t be necessary')
@click.option('--batch-size', type=int, default=1, show_default=True, help='Batch size (an image is scored over the anchors of its padded batch)')
@click.option('--dataloader-workers', type=int, default=4, show_default=True, help='Number of data loading threads (0 = read in the calling thread)')
@click.argument('state-file', type=click.Path(**_FILE))
def seek_sku110k_outliers(imgs, annotations, outlier_threshold, trim_module_prefix, batch_size, dataloader_workers, state_file):
    """Pass SKU110K data through GLN, print outliers.

    Every image that is not in the skip list is scored by the three losses of the reference's compute_loss -- classification,
    bbox_regression, gaussian -- on the GPU, in one pass over the data with one copy back at the end; images with a
    loss more than --outlier-threshold standard deviations above its average are printed.  Eval-mode statistics, no flips
    (INTEGRATION.md)."""
    from .. import device_gaussians, device_headloss
    data = datautils.SKU110KDataset(imgs, annotations, skip=SKU110K_SKIP, include_gaussians=False, flip_chance=0, image_format='uint8')
    model = proposals_eval.load_gln(state_file, trim_module_prefix)
    head_score = device_headloss.HeadScore(model, outlier_threshold=outlier_threshold)
    gaussian_score = device_gaussians.GaussianScore(model, outlier_threshold=outlier_threshold)
    model.keep_head_outputs(True)
    done = 0
    with torch.no_grad():
        for batch in proposals_eval._batches(feeding.feed(data, dataloader_workers), batch_size):
            if done % 200 < len(batch):
                print(f'{done - done % 200}...')
            done += len(batch)
            sizes = [datautils.image_hw(img) for img, _ in batch]
            result = model([img.cuda(non_blocking=True) for img, _ in batch])
            head_score.update(model.head_outputs(), [t for _, t in batch], sizes)
            gaussian_score.update(result, [t['boxes'] for _, t in batch], sizes)
    scored = device_headloss.compute_together(head_score, gaussian_score)
    names = ('classification', 'bbox_regression', 'gaussian')
    print('-' * 10)
    print('Mean loss:\t' + '\t'.join(str(scored[k]['mean']) for k in names))
    print('Std loss:\t' + '\t'.join(str(scored[k]['std']) for k in names))
    print('-' * 10)
    outliers = sorted(set().union(*(scored[k]['outliers'] for k in names)))
    if not outliers:
        print('No outliers! Have a nice day!')
    for i in outliers:
        print(f'Outlier at index {i}: {data.index[i]["image_name"]}')
        print('\t' + '\t'.join(str(float(scored[k]['loss'][i])) for k in names))


@gln.command()
@click.option('--conf-thresh', type=float, default=0.5, show_default=True, help='Confidence threhsold for detections')
@click.option('--save', type=click.Path(writable=True), help='Path to save the resulting image to')
@click.argument('state-file', type=click.Path(**_FILE))
@click.argument('image-file', type=click.Path(**_FILE))
def detect(conf_thresh, save, state_file, image_file):
    """Detect products; prints the boxes (x1 y1 x2 y2) and, with --save, writes the image with the boxes drawn."""
    from PIL import Image, ImageDraw
    model = proposals.gln(pretrained_backbone=False).cuda()
    model.load_state_dict(torch.load(state_file, map_location='cpu')[MODEL_STATE_DICT_KEY])
    model.eval()
    generator = production.ProposalGenerator(model, confidence_threshold=conf_thresh)
    pil_img = Image.open(image_file).convert('RGB')
    with torch.no_grad():
        detections = generator.generate_proposals(datautils.pil_to_uint8(pil_img)).cpu()
    for x1, y1, x2, y2 in detections.tolist():
        print(f'{x1:.1f} {y1:.1f} {x2:.1f} {y2:.1f}')
    print(f'--> {len(detections)} detections')
    if save is not None:
        draw = ImageDraw.Draw(pil_img)
        for box in detections.tolist():
            draw.rectangle(box, outline=(0, 255, 0), width=3)
        pil_img.save(save)


# ------------------------------------------------------------------ dihe -----------------------------------------------
@cli.group()
def dihe():
    """Product classification (DIHE embedder)."""


@dihe.command(name='eval', cls=_DeviceEvalCommand)
@click.option('--img-dir', type=click.Path(**_DIR), multiple=True, default=GP_TRAIN_FOLDERS, show_default=True,
              help='Path to GP training image root')
@click.option('--test-imgs', type=click.Path(**_DIR), default=GP_TEST_DIR, show_default=True, help='Path to GP test image root')
@click.option('--annotations', type=click.Path(**_DIR), default=GP_ANN_DIR, show_default=True, help='Path to GP-180 annotation root')
@click.option('--model', type=click.Choice(('vgg16', 'resnet50')), default='vgg16', show_default=True, help='Base for the encoder model')
@click.option('--resnet-layers', type=int, multiple=True, default=[2, 3], show_default=True, help='(resnet50 only)')
@click.option('--batch-norm/--no-batch-norm', default=False, show_default=True, help="Use/don't use batch normalization in encoder")
@click.option('--batch-size', type=int, default=8, show_default=True, help='Batch size')
@click.option('--dataloader-workers', type=int, default=8, show_default=True, help='Number of data loading threads (0 = read in the calling thread)')
@click.option('--enc-weights', help='Path to encoder weights')
@click.option('--only', type=click.Choice(('none', 'test', 'val')), default='none', show_default=True,
              help='Use all images (none) or only the test- or validation split')
@click.option('--knn', type=int, multiple=True, default=(1,), show_default=True,
              help='Consider classification correct if the correct class is among this many closest neighbours')
def dihe_eval(img_dir, test_imgs, annotations, model, resnet_layers, batch_norm, batch_size, dataloader_workers, enc_weights,
              only, knn):
    """Evaluate classification performance."""
    if enc_weights is None:
        raise click.UsageError('--enc-weights is required: ImageNet weights cannot be downloaded here')
    if model == 'vgg16':
        encoder = classification.macvgg_embedder(model='vgg16_bn' if batch_norm else 'vgg16', pretrained=False).cuda()
    else:
        encoder = classification.macresnet_encoder(pretrained=False, desc_layers=list(resnet_layers)).cuda()
    encoder.load_state_dict(torch.load(enc_weights, map_location='cpu')[EMBEDDER_STATE_DICT_KEY])
    encoder.eval().requires_grad_(False)
    sampleset = datautils.GroceryProductsDataset(img_dir, include_annotations=True, image_format='uint8')
    only_list = skip_list = None
    if only == 'test':
        skip_list = GP_TEST_VALIDATION_SET_SIZE
    elif only == 'val':
        only_list = GP_TEST_VALIDATION_SET_SIZE
    testset = datautils.GroceryProductsTestSet(test_imgs, annotations, only=only_list, skip=skip_list, image_format='uint8')
    accuracy = classification_eval.eval_dihe(encoder, sampleset, testset, batch_size, dataloader_workers, k=knn, verbose=True,
                                             device_eval=_device_eval_switch(), window=EVAL_WINDOW)
    print(f'--> accuracy {accuracy}')


@dihe.command()
@click.option('--img-dir', type=click.Path(**_DIR), multiple=True, default=GP_TRAIN_FOLDERS, show_default=True,
              help='Path to training image root')
@click.option('--datatype', type=click.Choice(('gp', 'internal')), default='gp', show_default=True,
              help='Dataset type; gp for Grocery Product, internal for our internal dataset')
@click.option('--out-dir', type=click.Path(exists=True, file_okay=False, dir_okay=True, writable=True), default=OUT_DIR,
              show_default=True, help='Output directory for embedded images')
@click.argument('dihe-state', type=click.Path(**_FILE))
def prebuild_index(img_dir, datatype, out_dir, dihe_state):
    """Pre-embed images.

    Passes all the images in the training set through the encoder and saves the resulting embedding vectors
    (classifier_index.pkl, usable with --load-classifier-index)."""
    sampleset = (datautils.GroceryProductsDataset(img_dir, include_annotations=True, image_format='uint8') if datatype == 'gp'
                 else datautils.InternalTrainSet(img_dir[0], include_annotations=True, image_format='uint8'))
    classifier = production.Classifier(_load_encoder(dihe_state), sampleset, verbose=True)
    classifier.save_index(os.path.join(out_dir, 'classifier_index.pkl'))


# ------------------------------------------------------------------ whole pipeline -------------------------------------
@cli.command(cls=_DeviceMetricsCommand)
@click.option('--img-dir', type=click.Path(**_DIR), multiple=True, default=GP_TRAIN_FOLDERS, show_default=True,
              help='Path to GP training image root')
@click.option('--test-imgs', type=click.Path(**_DIR), default=GP_TEST_DIR, show_default=True, help='Path to GP test image root')
@click.option('--annotations', type=click.Path(**_DIR), default=GP_ANN_DIR, show_default=True, help='Path to GP-180 annotation root')
@click.option('--iou-threshold', '-t', type=float, multiple=True, default=(0.5,), show_default=True,
              help='IoU thresholds to calculate metrics for')
@click.option('--coco/--no-coco', default=False, show_default=True,
              help="Whether to use COCO IoU thresholds instead of whatever's set in --iou-threshold")
@click.option('--load-classifier-index', type=click.Path(),
              help='Load pre-embedded images from given path instead of calculating the embedding on the fly')
@click.argument('gln-state', type=click.Path(**_FILE))
@click.argument('dihe-state', type=click.Path(**_FILE))
def eval_product_detection(img_dir, test_imgs, annotations, iou_threshold, coco, load_classifier_index, gln_state, dihe_state):
    """Evaluate product detection performance."""
    dataloader_workers = _reader_threads()
    sampleset = datautils.GroceryProductsDataset(img_dir, include_annotations=True, image_format='uint8')
    testset = datautils.GroceryProductsTestSet(test_imgs, annotations, retinanet_annotations=True, image_format='uint8')
    thresholds = _coco_or(iou_threshold, coco)
    proposal_generator = proposals_eval.load_gln(gln_state, False, detections_per_img=200)
    proposal_generator.requires_grad_(False)
    res, all_res = detection_eval.evaluate_detections(proposal_generator, _load_encoder(dihe_state), testset, sampleset,
                                                      thresholds=thresholds, num_workers=dataloader_workers,
                                                      load_classifier_index=load_classifier_index, device_metrics=_device_metrics_switch())
    mam = detection_eval.mean_average_metrics(res, thresholds)
    m_ap = m_ar = 0
    for t in thresholds:
        print(t, all_res[t])
        print(t, mam[t])
        m_ap += mam[t]['map']
        m_ar += mam[t]['mar300']
    print(f'--> mAP {m_ap / len(thresholds)}')
    print(f'--> mAR300 {m_ar / len(thresholds)}')


def _plano_sets(datatype, img_dir, test_imgs, test_annotations, planograms):
    if datatype == 'gp':
        return (datautils.PlanogramTestSet(test_imgs, test_annotations, planograms, image_format='uint8'),
                datautils.GroceryProductsDataset(img_dir, include_annotations=True, image_format='uint8'))
    return datautils.InternalPlanoSet(planograms, image_format='uint8'), datautils.InternalTrainSet(img_dir[0], include_annotations=True, image_format='uint8')


def _plano_evaluator(gln_state, dihe_state, sampleset, load_classifier_index, graph_threshold=0.5):
    proposal_generator = proposals_eval.load_gln(gln_state, False)
    proposal_generator.requires_grad_(False)
    generator = production.ProposalGenerator(proposal_generator)
    classifier = production.Classifier(_load_encoder(dihe_state), sampleset, batch_size=8, load=load_classifier_index)
    return production.PlanogramEvaluator(generator, classifier, production.PlanogramComparator(graph_threshold=graph_threshold,
                                                                                          device_graphs=_device_graphs_switch(),
                                                                                          device_tail=_device_tail_switch(),
                                                                                          device_reclass=_device_reclass_switch(),
                                                                                          matcher=_matcher_name()),
                                         device_detections=_device_detections_switch())


def _scene_renderer(evaluator, sampleset, workers, **atlas_options):
    """the gallery's product images on the device, row by row the classifier's, and the compositor over them"""
    from .. import rendering
    atlas = rendering.ThumbnailAtlas(sampleset, evaluator.classifier.annotations, evaluator.proposal_generator.device, num_workers=workers,
                                     **atlas_options)
    return rendering.SceneRenderer(atlas)


def _accuracy_line(acc, plano):
    err = acc - plano['actual_accuracy']
    return f'Detected accuracy: {acc:.3f}, Actual accuracy: {plano["actual_accuracy"]:.3f}, Error: {err:.3f}, SE: {err ** 2:.3f}'


@cli.command(cls=_DeviceDetectionsCommand)
@click.option('--img-dir', type=click.Path(**_DIR), multiple=True, default=GP_TRAIN_FOLDERS, show_default=True,
              help='Path to training image root')
@click.option('--test-imgs', type=click.Path(**_DIR), default=GP_TEST_DIR, show_default=True, help='Path to test image root')
@click.option('--test-annotations', type=click.Path(**_DIR), default=GP_ANN_DIR, show_default=True, help='Path to annotation root')
@click.option('--planograms', type=click.Path(**_DIR), default=GP_PLANO_DIR, show_default=True, help='Path to planograms root')
@click.option('--datatype', type=click.Choice(('gp', 'internal')), default='gp', show_default=True,
              help='Dataset type; gp for Grocery Product, internal for our internal dataset')
@click.option('--load-classifier-index', type=click.Path(),
              help='Load pre-embedded images from given path instead of calculating the embedding on the fly')
@click.option('--plano-idx', type=int, default=0, show_default=True, help='Rebuild the image with the given index')
@click.option('--out', type=click.Path(writable=True), required=True,
              help='Prefix of the pictures: PREFIX_annotated.png, PREFIX_observed.png and PREFIX_expected.png are written')
@click.argument('gln-state', type=click.Path(**_FILE))
@click.argument('dihe-state', type=click.Path(**_FILE))
def rebuild_scene(img_dir, test_imgs, test_annotations, planograms, datatype, load_classifier_index, plano_idx, out, gln_state, dihe_state):
    """Rebuild scene from product detections.

    Writes the shelf image with the compliance report drawn on it, the observed planogram (every detection's product image where it
    was detected) and the expected planogram rebuilt the same way, and prints the compliance."""
    planoset, sampleset = _plano_sets(datatype, img_dir, test_imgs, test_annotations, planograms)
    if not 0 <= plano_idx < len(planoset):
        raise click.UsageError(f'--plano-idx {plano_idx}: the set has {len(planoset)} images')
    evaluator = _plano_evaluator(gln_state, dihe_state, sampleset, load_classifier_index)
    renderer = _scene_renderer(evaluator, sampleset, _reader_threads())
    d = planoset[plano_idx]
    img, plano = (d[0], d[3]) if datatype == 'gp' else tuple(d)
    report, pictures = evaluator.pictures(img, plano, renderer)
    for path in pictures.save(out):
        print(path)
    print(_accuracy_line(float(report.compliance), plano))


@cli.command(cls=_MatcherCommand)
@click.option('--img-dir', type=click.Path(**_DIR), multiple=True, default=GP_TRAIN_FOLDERS, show_default=True,
              help='Path to training image root')
@click.option('--test-imgs', type=click.Path(**_DIR), default=GP_TEST_DIR, show_default=True, help='Path to test image root')
@click.option('--test-annotations', type=click.Path(**_DIR), default=GP_ANN_DIR, show_default=True, help='Path to annotation root')
@click.option('--planograms', type=click.Path(**_DIR), default=GP_PLANO_DIR, show_default=True, help='Path to planograms root')
@click.option('--datatype', type=click.Choice(('gp', 'internal')), default='gp', show_default=True,
              help='Dataset type; gp for Grocery Product, internal for our internal dataset')
@click.option('--load-classifier-index', type=click.Path(),
              help='Load pre-embedded images from given path instead of calculating the embedding on the fly')
@click.option('--verbose/--no-verbose', default=False, show_default=True, help='Print more information')
@click.argument('gln-state', type=click.Path(**_FILE))
@click.argument('dihe-state', type=click.Path(**_FILE))
def eval_planograms(img_dir, test_imgs, test_annotations, planograms, datatype, load_classifier_index, verbose, gln_state,
                    dihe_state):
    """Evaluate planogram compliance evaluation."""
    dataloader_workers = _reader_threads()
    planoset, sampleset = _plano_sets(datatype, img_dir, test_imgs, test_annotations, planograms)
    evaluator = _plano_evaluator(gln_state, dihe_state, sampleset, load_classifier_index)
    generator = evaluator.proposal_generator
    render_dir = _render_dir()
    renderer = None
    if render_dir:
        os.makedirs(render_dir, exist_ok=True)
        renderer = _scene_renderer(evaluator, sampleset, dataloader_workers)
    report_path = _report_file()
    report_out = open(report_path, 'w') if report_path else None
    total_a = total_e = 0.0
    # the reference evaluates one image at a time (cvpce/cli/eval.py:224-230); here the images are decoded ahead by the feeder's threads,
    # and EVAL_WINDOW of them are detected / embedded / matched together (PlanogramEvaluator.evaluate_batch: same per-image results,
    # one pass of the kernels per window)
    for s, data in enumerate(proposals_eval._batches(feeding.feed(planoset, dataloader_workers, generator.device), EVAL_WINDOW)):
        s *= EVAL_WINDOW
        pairs = [((d[0], d[3]) if datatype == 'gp' else tuple(d)) for d in data]
        if report_out is None and renderer is None:
            accs = evaluator.evaluate_batch([img for img, _ in pairs], [plano for _, plano in pairs])
        else:                                    # (the same route with its reasons: `.compliance` is evaluate_batch's value)
            if renderer is None:
                reports = evaluator.report_batch([img for img, _ in pairs], [plano for _, plano in pairs])
            else:                                # (and with its pictures: one launch per window, then a host encode per file)
                results = evaluator.pictures_batch([img for img, _ in pairs], [plano for _, plano in pairs], renderer)
                reports = [rep for rep, _ in results]
                for i, (_, pictures) in enumerate(results, start=s):
                    pictures.save(os.path.join(render_dir, str(i)))
            for i, rep in enumerate(reports, start=s) if report_out is not None else ():
                report_out.write(json.dumps(dict(rep.to_dict(), image=i)) + '\n')
            accs = [rep.compliance for rep in reports]
        for i, ((img, plano), acc) in enumerate(zip(pairs, accs), start=s):
            acc = float(acc)
            err = acc - plano['actual_accuracy']
            if verbose:
                print(_accuracy_line(acc, plano))
            elif i % 10 == 0:
                print(i)
            total_e += err ** 2
            total_a += acc
    if report_out is not None:
        report_out.close()
    print(f'--> Mean accuracy {total_a / len(planoset)}')
    print(f'--> MSE: {total_e / len(planoset)}')


_STEP_NAMES = 'detections, positions, expected_graph, observed_graph, expected_matched, observed_matched, annotated, observed and expected'


@cli.command(cls=_DeviceDetectionsCommand)
@click.option('--img-dir', type=click.Path(**_DIR), multiple=True, default=GP_TRAIN_FOLDERS, show_default=True,
              help='Path to training image root')
@click.option('--test-imgs', type=click.Path(**_DIR), default=GP_TEST_DIR, show_default=True, help='Path to test image root')
@click.option('--test-annotations', type=click.Path(**_DIR), default=GP_ANN_DIR, show_default=True, help='Path to annotation root')
@click.option('--planos', type=click.Path(**_DIR), default=GP_PLANO_DIR, show_default=True, help='Path to planograms root')
@click.option('--datatype', type=click.Choice(('gp', 'internal')), default='gp', show_default=True,
              help='Dataset type; gp for Grocery Product, internal for our internal dataset')
@click.option('--load-classifier-index', type=click.Path(),
              help='Load pre-embedded images from given path instead of calculating the embedding on the fly')
@click.option('--plano-idx', type=int, help='Visualize image with given index instead of choosing randomly')
@click.option('--out', type=click.Path(writable=True), required=True,
              help=f'Prefix of the pictures: PREFIX_<name>.png is written for {_STEP_NAMES}')
@click.argument('gln-state', type=click.Path(**_FILE))
@click.argument('dihe-state', type=click.Path(**_FILE))
def plot_planogram_eval(img_dir, test_imgs, test_annotations, planos, datatype, load_classifier_index, plano_idx, out, gln_state, dihe_state):
    """Visualize planogram compliance evaluation steps.

    Does the proposed planogram compliance evaluation procedure step by step and writes a picture for each step: the detections and
    the projected expected positions on the shelf image, the neighbour graphs and the matched common subgraph drawn over the rebuilt
    expected and observed planograms, and the pictures of rebuild-scene.  Prints the compliance."""
    import random
    planoset, sampleset = _plano_sets(datatype, img_dir, test_imgs, test_annotations, planos)
    if plano_idx is None:
        plano_idx = random.randrange(len(planoset))
    if not 0 <= plano_idx < len(planoset):
        raise click.UsageError(f'--plano-idx {plano_idx}: the set has {len(planoset)} images')
    evaluator = _plano_evaluator(gln_state, dihe_state, sampleset, load_classifier_index)
    renderer = _scene_renderer(evaluator, sampleset, _reader_threads())
    d = planoset[plano_idx]
    img, plano = (d[0], d[3]) if datatype == 'gp' else tuple(d)
    report, pictures = evaluator.step_pictures(img, plano, renderer)
    for path in pictures.save(out):
        print(path)
    print(_accuracy_line(float(report.compliance), plano))


@cli.group()
def misc():
    """Miscellaneous commands."""


PIPELINE_DEMO_GRAPH_THRESHOLD = 0.7       # cli/misc.py:177-178


@misc.command(cls=_DeviceDetectionsCommand)
@click.option('--out', type=click.Path(writable=True), required=True,
              help=f'Prefix of the pictures: PREFIX_<name>.png is written for {_STEP_NAMES}')
@click.option('--scale-gallery/--no-scale-gallery', default=False, show_default=True,
              help='Embed the product photos in [-1, 1] (scale_to_tanh), the range the encoder sees its queries in.  Off, the default, '
                   'is what the reference does: it embeds this gallery in [0, 1] although the queries are in [-1, 1].')
@click.argument('gln-state', type=click.Path(**_FILE))
@click.argument('dihe-state', type=click.Path(**_FILE))
@click.argument('dataset-folder', type=click.Path(**_DIR))
@click.argument('image-file', type=click.Path(**_FILE))
@click.argument('plano-file', type=click.Path(**_FILE))
def pipeline_demo(out, scale_gallery, gln_state, dihe_state, dataset_folder, image_file, plano_file):
    """Demonstrate the CVPCE pipeline.

    The dataset folder is expected to contain .png, .jpg and .jpeg files,
    one for each class, with the class label set as the filename.

    The planogram file should be a JSON file formatted in a manner such as

    \b
    [
        {
            "label": "class1",
            "box": [0, 0, 5, 5]
        },
        {
            "label": "class2",
            "box": [5, 0, 10, 5]
        }
    ]

    (in this case, the dataset folder should contain files for class1 and class2,
    such as class1.png and class2.jpg)

    Writes the step pictures of plot-planogram-eval and prints the compliance.  The two embedding scatter plots of the reference's
    demo are not drawn."""
    dataset = datautils.SimpleFolderSet(dataset_folder, scale=scale_gallery)
    rebuildset = datautils.SimpleFolderSet(dataset_folder, train=False)
    if not len(dataset):
        raise click.UsageError(f'{dataset_folder} holds no .png, .jpg or .jpeg file')
    evaluator = _plano_evaluator(gln_state, dihe_state, dataset, None, graph_threshold=PIPELINE_DEMO_GRAPH_THRESHOLD)
    renderer = _scene_renderer(evaluator, rebuildset, _reader_threads(), float_items='unit')
    img = datautils._image_reader('uint8')(datautils._open_image(image_file))
    plano = datautils.read_planogram_json(plano_file)
    report, pictures = evaluator.step_pictures(img, plano, renderer)
    for path in pictures.save(out):
        print(path)
    print(f'Compliance: {float(report.compliance):.3f} ({report.status})')


if __name__ == '__main__':
    cli()
