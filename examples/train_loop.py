"""Minimal end-to-end training loop on munit_amd: the loaders of munit_amd.data feeding MUNIT_Trainer, in the
shape of the reference's scripts/train.py:157-330 (dis_update / gen_update cadence of `ratio_disc_gen`,
update_learning_rate first, periodic sample grids, periodic save, periodic FID).  Control plane only -- no comet.

  python examples/train_loop.py --config configs.yaml --data-root /path/with/trainA,trainB,testA,testB [--iters N]
  torchrun --nproc-per-node 8 --master-addr 127.0.0.1 examples/train_loop.py ...      (data parallel, RCCL)

The synthetic-pair iteration of scripts/train.py:229-260 runs every `synthetic_frequency` iterations when the five lists
of munit_amd.data.get_synthetic_data_loader are given: --synth-list-a, --synth-list-b, --synth-mask-list, --seg-list-a and
--seg-list-b, each falling back to the config key the reference reads (data_list_train_a_synth, data_list_train_b_synth,
data_list_train_b_seg_synth, seg_list_a, seg_list_b; scripts/train.py:104-117) when that file exists.  The loader is
restarted when it runs out.  Called from Python, main() also takes `synth_pairs`, an iterator of
(x_as, x_bs, mask_s, sem_a, sem_b) batches, which then takes precedence (sem_a / sem_b may be None, the reference's
`synthetic_seg_gt: 0`).  Without the lists and without `synth_pairs` no synthetic iteration runs.

Output-level adaptation (adaptation.output_classifier_lambda and output_adv_lambda): every `output_classif_freq` iterations
output_domain_classifier_sr_update runs on (x_a, x_as, x_b, x_bs), scripts/train.py:209-223, with the synthetic batch of
that iteration (the one its synthetic-pair step uses too, when both fall on the same iteration).  A trainer that owns these
classifiers cannot train without synthetic images: without the lists (or `synth_pairs`) the loop stops at start-up.

With --output-path the folder gets the reference's layout (munit_amd.utils.prepare_sub_folder): checkpoints/ and images/.  The
sample grids of scripts/train.py:285-320 are written into images/: `display_size` samples of each train loader (and of each
test loader -- testA / testB under the data root, or the config's data_folder_test_* / data_list_test_* -- when those exist)
are taken once before the first iteration; every `image_save_iter` iterations gen_a2b_ / gen_b2a_test_%08d.jpg and
..._train_%08d.jpg are written, every `image_display_iter` iterations ..._train_current.jpg (write_samples; a key that is
absent or 0 writes nothing).  All ranks sample -- sample() draws styles from the host RNG -- and rank 0 writes.  Checkpoints
(--save-every) go to checkpoints/ unless --output names another folder; --output alone keeps its meaning, a bare checkpoint
folder and no grids.

FID (--fid-every N, default 0): the reference builds get_inception_metrics when `eval_fid` > 0 (scripts/train.py:119-130) but
never calls it in its loop, so the cadence is this script's.  With eval_fid > 0 and N > 0 the FID loader
(data_list_fid_a / data_list_fid_b, batch_size_fid) and prepare_inception_metrics(inception_moment_path) are built as the
reference does -- the Inception weights come from the file MUNIT_INCEPTION_CKPT names -- and rank 0 evaluates and prints `FID`
after every N-th iteration.
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


SYNTH_LISTS = (("synth_list_a", "data_list_train_a_synth"), ("synth_list_b", "data_list_train_b_synth"),
               ("synth_mask_list", "data_list_train_b_seg_synth"), ("seg_list_a", "seg_list_a"), ("seg_list_b", "seg_list_b"))


def synth_lists(args, config):
    """The five list files of the synthetic loader, or None when one is missing: the command line first, then the config
    key when the file it names exists."""
    out = []
    for arg, key in SYNTH_LISTS:
        f = getattr(args, arg)
        if not f and isinstance(config.get(key), str) and os.path.isfile(config[key]):
            f = config[key]
        if not f:
            return None
        out.append(f)
    return out


def restarting(loader):
    """Batches of `loader` for ever: a new epoch (new order, new draws) whenever it runs out."""
    while True:
        n = 0
        for batch in loader:
            n += 1
            yield batch
        if n == 0:
            raise RuntimeError("the synthetic loader yields no batch (fewer samples than one batch)")


def run_iteration(trainer, config, it, real_batch, synth_pairs, on_call=None):
    """Iteration `it` (counted from 0) in the order scripts/train.py:172-274 issues it: update_learning_rate, the real
    dis_update, a gen_update when (it + 1) % ratio_disc_gen == 0, the classifier updates on their own cadences of it + 1,
    then -- when it % synthetic_frequency == 0 -- a synthetic dis_update, a gen_update(synth=True) that ratio_disc_gen does
    not gate, and the synthetic feature-classifier update; last, in every iteration with synthetic_frequency > 0, the
    segmentation_head_update of a trainer with train_seg (scripts/train.py:275-283).  real_batch: (x_a, x_b, mask_a, mask_b); synth_pairs: an iterator
    of (x_as, x_bs, mask_s, sem_a, sem_b) or None.  on_call(name, args, run): called in place of every update with the
    trainer method's name, its positional arguments and `run`, which performs the call (tests wrap the calls with it)."""
    def call(name, *args):
        run = lambda: getattr(trainer, name)(*args)
        return run() if on_call is None else on_call(name, args, run)

    x_a, x_b, m_a, m_b = real_batch
    ad = config["adaptation"]
    trainer.iterations = it
    trainer.update_learning_rate()
    call("dis_update", x_a, x_b, config)                                # scripts/train.py:182
    if (it + 1) % int(config.get("ratio_disc_gen", 1)) == 0:
        call("gen_update", x_a, x_b, config, m_a, m_b)                  # scripts/train.py:185-187
    cls_due = trainer.use_classifier_sr and (it + 1) % ad["classif_frequency"] == 0
    if cls_due:                                                         # scripts/train.py:193-207: real codes, target 1
        call("domain_classifier_sr_update", x_a, x_b, False, ad["dfeat_lambda"], it + 1)
    pair = None
    if trainer.use_output_classifier_sr and (it + 1) % ad["output_classif_freq"] == 0:
        pair = next(synth_pairs)                                        # scripts/train.py:209-223: real a, synthetic a, real b, synthetic b
        call("output_domain_classifier_sr_update", x_a, pair[0], x_b, pair[1], config, it + 1)
    freq = int(config.get("synthetic_frequency", 0))
    if synth_pairs is not None and freq > 0 and it % freq == 0:         # scripts/train.py:229-260
        pair = pair if pair is not None else next(synth_pairs)
        x_as, x_bs, mask_s, sem_a, sem_b = pair
        if config.get("synthetic_seg_gt", 0) == 0:
            sem_a = sem_b = None
        call("dis_update", x_as, x_bs, config)
        call("gen_update", x_as, x_bs, config, mask_s, mask_s, None, True, sem_a, sem_b)
        if cls_due:                                                     # scripts/train.py:261-274: synthetic codes, target 0
            call("domain_classifier_sr_update", x_as, x_bs, True, ad["dfeat_lambda"], it + 1)
    if synth_pairs is not None and freq > 0 and getattr(trainer, "train_seg", False):
        # scripts/train.py:275-283: in every iteration, on the iteration's synthetic pair (the one the steps above used when
        # they ran; the reference's loop loads a pair in every iteration) and its label maps, whatever synthetic_seg_gt says
        x_as, x_bs, _, sem_a, sem_b = pair if pair is not None else next(synth_pairs)
        call("segmentation_head_update", x_as, x_bs, sem_a, sem_b, ad["sem_seg_lambda"], None)


def display_batch(loader, display_size):
    """scripts/train.py:132-143: the first `display_size` samples of the loader's dataset as one batch (the image of a
    loader that yields (image, mask) pairs)."""
    items = [loader.dataset[i] for i in range(display_size)]
    return torch.stack([t[0] if isinstance(t, tuple) else t for t in items])


def held_out_loaders(config, root, batch, new_size, num_workers):
    """The two test loaders as munit_amd.data.get_all_data_loaders builds them (new_size is the crop as well, no shuffle,
    no flip) when their files exist, else None."""
    from munit_amd import data as D
    out = []
    for dom in ("a", "b"):
        folder = os.path.join(root, "test" + dom.upper()) if root else None
        flist, froot = config.get("data_list_test_" + dom), config.get("data_folder_test_" + dom)
        if folder and os.path.isdir(folder) and D.make_dataset(folder):
            out.append(D.get_data_loader_folder(folder, batch, False, new_size, new_size, new_size, num_workers, seed=4))
        elif isinstance(flist, str) and isinstance(froot, str) and os.path.isfile(flist):
            out.append(D.get_data_loader_list(froot, flist, batch, False, new_size, new_size, new_size, num_workers, seed=4))
        else:
            return None
    return out


def write_samples(trainer, config, it, displays, image_directory, rank=0, write=None, comet_exp=None):
    """The sample grids of iteration `it` (counted from 0), scripts/train.py:285-320: when (it + 1) % image_save_iter == 0
    the test pair and the train pair are sampled, in that order, and written as test_%08d and train_%08d; when
    (it + 1) % image_display_iter == 0 the train pair is sampled again and written as train_current.  A cadence key that
    is absent or 0 writes nothing.  displays: (train_a, train_b, test_a, test_b) display batches, the test pair None when
    there are no test images (then only the train grids are written).  Every rank samples -- sample() draws its random
    styles from the host RNG, which has to advance alike on all ranks -- and rank 0 alone calls
    write(outputs, display_size, image_directory, postfix, comet_exp) (default: munit_amd.utils.write_2images)."""
    if write is None:
        from munit_amd.utils import write_2images as write
    train_a, train_b, test_a, test_b = displays
    n = config["display_size"]
    save_every = int(config.get("image_save_iter") or 0)
    show_every = int(config.get("image_display_iter") or 0)
    if save_every > 0 and (it + 1) % save_every == 0:
        with torch.no_grad():
            test_outputs = trainer.sample(test_a, test_b) if test_a is not None else None
            train_outputs = trainer.sample(train_a, train_b)
        if rank == 0:
            if test_outputs is not None:
                write(test_outputs, n, image_directory, "test_%08d" % (it + 1), comet_exp)
            write(train_outputs, n, image_directory, "train_%08d" % (it + 1), comet_exp)
    if show_every > 0 and (it + 1) % show_every == 0:
        with torch.no_grad():
            outputs = trainer.sample(train_a, train_b)
        if rank == 0:
            write(outputs, n, image_directory, "train_current", comet_exp)


def fid_due(config, it, every):
    """Whether iteration `it` (counted from 0) ends with an FID evaluation: eval_fid > 0 in the config, --fid-every N > 0,
    and it + 1 a multiple of N."""
    return int(config.get("eval_fid") or 0) > 0 and int(every or 0) > 0 and (it + 1) % int(every) == 0


def build_fid(config):
    """(fid_loader factory, get_inception_metrics) as scripts/train.py:119-130 builds them."""
    from munit_amd import data as D
    from munit_amd.inception_utils import prepare_inception_metrics
    loader = lambda: D.get_fid_data_loader(config["data_list_fid_a"], config["data_list_fid_b"], config["batch_size_fid"],
                                           train=False, new_size=config["new_size"], num_workers=config.get("num_workers", 4))
    return loader, prepare_inception_metrics(inception_moment=config["inception_moment_path"], parallel=False)


def evaluate_fid(trainer, fid):
    """One FID evaluation with what build_fid returned: a fresh pass over the FID list, quietly; a Python float."""
    loader, get_inception_metrics = fid
    return get_inception_metrics(trainer, loader(), prints=False)


def main(argv=None, synth_pairs=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", required=True)
    ap.add_argument("--data-root", default=None, help="folder with trainA/ trainB/ testA/ testB (overrides the YAML lists)")
    ap.add_argument("--file-list-a"), ap.add_argument("--file-list-b")
    ap.add_argument("--mask-list-a"), ap.add_argument("--mask-list-b")
    ap.add_argument("--synth-list-a"), ap.add_argument("--synth-list-b"), ap.add_argument("--synth-mask-list")
    ap.add_argument("--seg-list-a"), ap.add_argument("--seg-list-b")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--output", default=None, help="checkpoint directory (default with --output-path: its checkpoints/)")
    ap.add_argument("--output-path", default=None, help="run folder in the reference's layout: checkpoints/ and images/ "
                    "are made inside it, and the sample grids are written")
    ap.add_argument("--save-every", type=int, default=0)
    ap.add_argument("--fid-every", type=int, default=0, help="with eval_fid > 0 in the config: rank 0 prints FID every N "
                    "iterations (0: never)")
    args = ap.parse_args(argv)

    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    dev = torch.device("cuda", local_rank)

    from munit_amd.utils import get_config, prepare_sub_folder
    from munit_amd.trainer import MUNIT_Trainer
    from munit_amd import data as D

    config = get_config(args.config)
    if "vgg_model_path" not in config and args.output_path:
        config["vgg_model_path"] = args.output_path      # scripts/train.py:62: vgg_w > 0 reads <it>/models/vgg16.weight
    torch.manual_seed(1234)                       # identical initial weights on every rank
    trainer = MUNIT_Trainer(config)
    trainer.to(dev)

    b, ns = config["batch_size"], config.get("new_size")
    h, w, nw = config["crop_image_height"], config["crop_image_width"], config.get("num_workers", 4)
    if args.mask_list_a:                          # scripts/train.py:80-100: image + mask loaders
        loader_a = D.get_data_loader_mask_and_im(args.file_list_a, args.mask_list_a, b, True, ns, h, w, nw, seed=1)
        loader_b = D.get_data_loader_mask_and_im(args.file_list_b, args.mask_list_b, b, True, ns, h, w, nw, seed=2)
    else:
        root = args.data_root or config["data_root"]
        loader_a = D.get_data_loader_folder(os.path.join(root, "trainA"), b, True, ns, h, w, nw, seed=1)
        loader_b = D.get_data_loader_folder(os.path.join(root, "trainB"), b, True, ns, h, w, nw, seed=2)

    if synth_pairs is None:                       # scripts/train.py:104-117: the synthetic paired loader
        lists = synth_lists(args, config)
        if lists is not None:
            synth_pairs = restarting(D.get_synthetic_data_loader(*lists, b, True, ns, h, w, nw, seed=3))

    if trainer.use_output_classifier_sr and synth_pairs is None:
        raise SystemExit("adaptation.output_classifier_lambda / output_adv_lambda train the output classifiers on synthetic "
                         "images: give the synthetic lists (%s, or the config keys %s)"
                         % (", ".join("--" + a.replace("_", "-") for a, _ in SYNTH_LISTS), ", ".join(k for _, k in SYNTH_LISTS)))

    checkpoint_directory, image_directory, displays = args.output, None, None
    if args.output and local_rank == 0:
        os.makedirs(args.output, exist_ok=True)
    if args.output_path:
        if local_rank == 0:
            sub, image_directory = prepare_sub_folder(args.output_path)
            checkpoint_directory = checkpoint_directory or sub
        # scripts/train.py:132-143, on every rank: dataset[i] draws from the loader's RNG, and the ranks' draws stay alike
        n = config["display_size"]
        tests = held_out_loaders(config, None if args.mask_list_a else (args.data_root or config.get("data_root")), b, ns, nw)
        displays = (display_batch(loader_a, n), display_batch(loader_b, n)) + \
            ((display_batch(tests[0], n), display_batch(tests[1], n)) if tests else (None, None))
    fid = None
    if int(config.get("eval_fid") or 0) > 0 and args.fid_every > 0 and local_rank == 0:
        fid = build_fid(config)
    it, t0 = 0, time.perf_counter()
    while it < args.iters:
        for batch_a, batch_b in zip(loader_a, loader_b):
            (x_a, m_a), (x_b, m_b) = [(t if isinstance(t, tuple) else (t, None)) for t in (batch_a, batch_b)]
            if m_a is None and config.get("recon_mask", 0) == 1:      # no mask files: everything counts
                m_a, m_b = torch.ones_like(x_a[:, :1]), torch.ones_like(x_b[:, :1])
            run_iteration(trainer, config, it, (x_a, x_b, m_a, m_b), synth_pairs)
            if displays is not None:
                write_samples(trainer, config, it, displays, image_directory, local_rank)
            if fid is not None and fid_due(config, it, args.fid_every):
                print("iteration %d  FID %.4f" % (it + 1, evaluate_fid(trainer, fid)))
            it += 1
            if checkpoint_directory and args.save_every and it % args.save_every == 0 and local_rank == 0:
                trainer.save(checkpoint_directory, it - 1)      # file names carry iterations + 1 (trainer.py:1337-1344)
            if it >= args.iters:
                break
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if local_rank == 0:
        print("iterations %d  %.1f ms/iter  loss_dis_total %.5f" % (it, 1e3 * dt / max(it, 1), float(trainer.loss_dis_total)))
    if world > 1:
        dist.destroy_process_group()
    return trainer


if __name__ == "__main__":
    main()
