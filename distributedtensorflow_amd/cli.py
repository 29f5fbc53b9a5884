"""``train.py`` — one CLI for every model x strategy combination.

Keeps the reference's flags and adds strategy selection:

    # reference mode: between-graph parameter-server cluster (run_mnist_distributed.py:164-182)
    python train.py --job_name=ps     --task_index=0 [--config config.json]
    python train.py --job_name=worker --task_index=0 [--sync_replicas]
    #   ... or the template's comma lists (templates/00_mnist_replica.py:80-83)
    python train.py --job_name=worker --task_index=1 --ps_hosts=h:2222 --worker_hosts=h:2223,h:2224

    # tf.distribute-style strategies (one process per GPU; --num_gpus N spawns them via
    # torch.distributed.run on 127.0.0.1, or launch under torchrun / TF_CONFIG yourself)
    python train.py --model mnist_mlp --strategy onedevice --device cpu      # BASELINE config 1
    python train.py --model resnet50 --strategy mirrored --num_gpus 8        # configs 2 / 3
    python train.py --model resnet50 --strategy ps --num_ps 1 --num_gpus 8   # config 4
    python train.py --model bert_base --strategy multiworker --num_gpus 8    # config 5
    # large-batch ResNet recipe: LARS + label smoothing + warm-up / polynomial decay
    python train.py --model resnet50 --num_gpus 8 --optimizer lars --learning_rate LR
                    --label_smoothing 0.1
    # loss / top-1 / top-k over all replicas: at the end (--eval) and every N steps (--eval_every)
    python train.py --model resnet50 --num_gpus 8 --eval --eval_steps 20 --eval_every 500
    # moving averages of the variables, evaluated next to the raw weights
    python train.py --model resnet50 --num_gpus 8 --ema_decay 0.9999 --eval
    # a left-to-right language model on a token set: causal attention, next-token targets
    python train.py --model bert_base --num_gpus 8 --text_data DIR --causal_lm --eval

The chief prints the reference's ``Worker (i): loss = x.xx (global step: n)`` line every
``--log_every`` steps and writes ``Global Step`` / ``Loss`` TensorBoard scalars under
``--log_dir/<timestamp>`` (``run_mnist_distributed.py:136-159``); ``--checkpoint_dir`` enables TF-V2
checkpoints + restore-on-restart through MonitoredTrainingSession.
"""
from __future__ import annotations

import argparse
import datetime
import json
import math
import os
import subprocess
import sys
import time

MODELS = ("mnist_cnn", "mnist_mlp", "resnet50", "resnet101", "resnet152", "bert_base",
          "bert_large")
STRATEGIES = ("onedevice", "mirrored", "multiworker", "ps")


def build_parser():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    # reference flags (run_mnist_distributed.py:167-180, templates/00_mnist_replica.py:49-84)
    p.add_argument("--job_name", default=None, help="ps | worker (between-graph cluster mode)")
    p.add_argument("--task_index", type=int, default=0)
    p.add_argument("--config", default="config.json", help="cluster JSON (ps / workers)")
    p.add_argument("--ps_hosts", default=None)
    p.add_argument("--worker_hosts", default=None)
    p.add_argument("--existing_servers", action="store_true",
                   help="attach to an already running cluster rendezvous (template R18)")
    p.add_argument("--sync_replicas", action="store_true")
    p.add_argument("--replicas_to_aggregate", type=int, default=None)
    p.add_argument("--num_gpus", type=int, default=None,
                   help="GPUs on this node (one process each); 0 = CPU")
    p.add_argument("--data_dir", default="/tmp/data/")
    p.add_argument("--download_only", action="store_true")
    p.add_argument("--hidden_units", type=int, default=100)
    p.add_argument("--train_steps", "--max_steps", dest="max_steps", type=int, default=1000)
    p.add_argument("--batch_size", type=int, default=None, help="per-replica batch")
    p.add_argument("--learning_rate", type=float, default=None)
    # framework flags
    p.add_argument("--model", choices=MODELS, default="mnist_cnn")
    p.add_argument("--strategy", choices=STRATEGIES, default=None)
    p.add_argument("--device", choices=("auto", "cpu", "gpu"), default="auto")
    p.add_argument("--optimizer",
                   choices=("adam", "adagrad", "momentum", "sgd", "lamb", "lars", "adamw"),
                   default=None,
                   help="lars: the large-batch ResNet recipe (needs --learning_rate); adamw: "
                        "BERT's AdamWeightDecayOptimizer (with --clip_norm 1.0 the BERT recipe)")
    p.add_argument("--clip_norm", type=float, default=None,
                   help="clip every step's gradient to this global norm, inside the fused update")
    p.add_argument("--accumulation_steps", type=int, default=1,
                   help="accumulate the gradients of N micro-batches per update (a global batch "
                        "of batch * replicas * N); steps, logging and hooks count updates")
    p.add_argument("--ema_decay", type=float, default=None,
                   help="keep tf.train.ExponentialMovingAverage(D, num_updates=global_step) of the "
                        "trainable variables inside the fused step; --eval / --eval_every then "
                        "also evaluate the averaged weights")
    p.add_argument("--label_smoothing", type=float, default=0.0,
                   help="label smoothing of the sparse softmax cross-entropy loss")
    p.add_argument("--num_ps", type=int, default=None, help="colocated PS owners (strategy ps)")
    p.add_argument("--variable_placement", choices=("balanced", "round_robin"),
                   default="balanced")
    p.add_argument("--bucket_mb", type=float, default=64)
    p.add_argument("--image_size", type=int, default=224)
    p.add_argument("--seq_len", type=int, default=128)
    p.add_argument("--log_dir", default="/tmp/distributed_logs")
    p.add_argument("--log_every", type=int, default=1)
    p.add_argument("--checkpoint_dir", default=None)
    p.add_argument("--save_checkpoint_steps", type=int, default=None)
    p.add_argument("--save_checkpoint_secs", type=int, default=600)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--eval", action="store_true",
                   help="evaluate at the end, over every replica: the MNIST test set, or "
                        "--eval_steps synthetic batches for ResNet / BERT")
    p.add_argument("--eval_every", type=int, default=0,
                   help="also evaluate every N global steps during training (0 = off)")
    p.add_argument("--eval_steps", type=int, default=10,
                   help="batches per replica of an evaluation on the synthetic sets")
    p.add_argument("--eval_top_k", type=int, default=5, help="k of the reported top-k accuracy")
    p.add_argument("--image_data", default=None, metavar="DIR",
                   help="train an image model on DIR/train_{images,labels}.npy (uint8 NHWC), kept "
                        "in device memory and augmented on the device; --eval / --eval_every "
                        "then evaluate on DIR/val_*.npy")
    p.add_argument("--augment", choices=("rrc", "pad_crop", "none"), default="rrc",
                   help="training transform with --image_data: random-resized-crop, pad 4 + "
                        "crop, or resize only (each with random flips)")
    p.add_argument("--mixup_alpha", type=float, default=0.0,
                   help="with --image_data: Mixup of each training batch inside the augmentation "
                        "kernel, blend weight ~ Beta(A, A); the loss becomes the two-label one")
    p.add_argument("--cutmix_alpha", type=float, default=0.0,
                   help="with --image_data: CutMix, box area share ~ Beta(A, A); with "
                        "--mixup_alpha too, each batch draws one of the two")
    p.add_argument("--randaugment", type=int, default=0, metavar="N",
                   help="with --image_data: RandAugment of each training example inside the "
                        "augmentation kernel, N layers (1 to 4; 0 = off)")
    p.add_argument("--ra_magnitude", type=float, default=9.0,
                   help="--randaugment: the magnitude, 0 to 10")
    p.add_argument("--ra_mstd", type=float, default=0.5,
                   help="--randaugment: standard deviation of the per-op magnitude noise")
    p.add_argument("--ra_prob", type=float, default=0.5,
                   help="--randaugment: the chance that a layer's op is applied")
    p.add_argument("--num_classes", type=int, default=None,
                   help="classes of the --image_data set (default: 1000 for ResNet, 10 for MNIST "
                        "models)")
    p.add_argument("--text_data", default=None, metavar="DIR",
                   help="train a BERT model on DIR/train_tokens.npy (uint16 / int32 [N, S]), kept "
                        "in device memory and masked on the device; the sequence length is the "
                        "file's; --eval / --eval_every then evaluate on DIR/val_tokens.npy")
    p.add_argument("--mlm_prob", type=float, default=0.15,
                   help="share of a row's tokens chosen for prediction with --text_data")
    p.add_argument("--max_predictions", type=int, default=20,
                   help="masked positions per example with --text_data")
    p.add_argument("--whole_word_mask", action="store_true",
                   help="with --text_data: whole-word masking (the pieces of a word are predicted "
                        "together), for training and evaluation; reads DIR/continuation.npy, "
                        "uint8 [vocab_size] with 1 at the ## pieces")
    p.add_argument("--causal_lm", action="store_true",
                   help="train a BERT model as a left-to-right language model: causal attention "
                        "in every layer, every position predicts the next token (pad excluded); "
                        "rows come from --text_data unmasked, or from the synthetic set; "
                        "--mlm_prob and --max_predictions are ignored; --eval / --eval_every "
                        "also report eval_perplexity, exp of the reported (4-place) eval_loss")
    return p


def check_data_args(args):
    """The data flags that cannot go together: a SystemExit names the offender."""
    if args.causal_lm:
        if not args.model.startswith("bert"):
            raise SystemExit(f"--causal_lm needs a BERT model, not {args.model}")
        if args.whole_word_mask:
            raise SystemExit("--causal_lm masks nothing: it cannot be combined with "
                             "--whole_word_mask")
    if args.text_data:
        if args.image_data:
            raise SystemExit("--text_data and --image_data cannot be combined")
        if not args.model.startswith("bert"):
            raise SystemExit(f"--text_data needs a BERT model, not {args.model}")
        if not 0.0 <= args.mlm_prob <= 1.0:
            raise SystemExit(f"--mlm_prob {args.mlm_prob} outside [0, 1]")
        if args.max_predictions < 1:
            raise SystemExit(f"--max_predictions {args.max_predictions} must be at least 1")
    if args.whole_word_mask:
        if not args.text_data:
            raise SystemExit("--whole_word_mask needs --text_data")
        table = os.path.join(args.text_data, "continuation.npy")
        if not os.path.exists(table):
            raise SystemExit(f"--whole_word_mask needs {table}")
    if args.mixup_alpha or args.cutmix_alpha:
        if args.mixup_alpha < 0 or args.cutmix_alpha < 0:
            raise SystemExit("--mixup_alpha and --cutmix_alpha must be >= 0")
        if args.model.startswith("bert") or args.model == "mnist_mlp":
            raise SystemExit(f"--mixup_alpha / --cutmix_alpha: {args.model} has no two-label loss")
        if not args.image_data:
            raise SystemExit("--mixup_alpha / --cutmix_alpha need --image_data")
    if args.randaugment:
        if args.model.startswith("bert"):
            raise SystemExit(f"--randaugment: {args.model} is not an image model")
        if not args.image_data:
            raise SystemExit("--randaugment needs --image_data")
        if not 1 <= args.randaugment <= 4:
            raise SystemExit("--randaugment takes 1 to 4 layers")
        if not 0 <= args.ra_magnitude <= 10 or args.ra_mstd < 0 or not 0 <= args.ra_prob <= 1:
            raise SystemExit("--ra_magnitude is in [0, 10], --ra_mstd >= 0, --ra_prob in [0, 1]")


DEFAULTS = {   # (batch, optimizer, learning rate) per model
    "mnist_cnn": (128, "adam", 5e-4),          # run_mnist_distributed.py:77,116
    "mnist_mlp": (100, "adam", 0.01),          # templates/00_mnist_replica.py:66-69
    "resnet50": (256, "momentum", 0.1),
    "resnet101": (256, "momentum", 0.1),
    "resnet152": (256, "momentum", 0.1),
    "bert_base": (128, "lamb", 1e-3),
    "bert_large": (64, "lamb", 1e-3),
}


def _spawn_local(args, argv):
    """--num_gpus N > 1 without a torch.distributed env: start N ranks as CHILD processes
    (torch.distributed.run on 127.0.0.1) and return their exit code.  Nothing in this parent
    process touches the GPU."""
    from .cluster.launcher import free_ports
    port = free_ports(1)[0]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           f"--nproc-per-node={args.num_gpus}", "--master-addr=127.0.0.1",
           f"--master-port={port}", os.path.abspath(sys.argv[0]), *argv]
    return subprocess.call(cmd)


def _make_optimizer(name, lr, model_name, batch_global, max_steps=None, clip_norm=None,
                    variable_averages=None, accumulation_steps=1):
    from . import optimizers as O
    from .optimizers.optimizers import cosine_decay, polynomial_decay
    kw = {} if clip_norm is None else {"clip_norm": clip_norm}
    if accumulation_steps > 1:
        kw["accumulation_steps"] = accumulation_steps
    if variable_averages is not None:
        kw["variable_averages"] = variable_averages
    if name == "adam":
        return O.AdamOptimizer(lr, **kw)
    if name == "adagrad":
        return O.AdagradOptimizer(lr, **kw)
    if name == "sgd":
        return O.GradientDescentOptimizer(lr, **kw)
    if name == "momentum":
        if model_name.startswith("resnet"):
            return O.MomentumOptimizer(cosine_decay(lr * batch_global / 256, 90 * 5000,
                                                    warmup_steps=500), 0.9, weight_decay=1e-4,
                                       **kw)
        return O.MomentumOptimizer(lr, 0.9, **kw)
    if name == "lamb":
        return O.LAMBOptimizer(polynomial_decay(lr, 10000, warmup_steps=100), weight_decay=0.01,
                               **kw)
    if name == "lars":
        # large-batch recipe: warm-up over the first 5% of the run, then polynomial (power 2)
        # decay to zero at the last step
        return O.LARSOptimizer(polynomial_decay(lr, max_steps, power=2,
                                                warmup_steps=max(1, max_steps // 20)),
                               0.9, weight_decay=1e-4, **kw)
    if name == "adamw":
        # google-research/bert: linear warm-up over the first 1% of the run, then linear decay
        # to zero at the last step
        return O.AdamWeightDecayOptimizer(
            polynomial_decay(lr, max_steps, warmup_steps=math.ceil(0.01 * max_steps)), **kw)
    raise ValueError(name)


def _cluster_from_args(args):
    from .cluster import ClusterSpec, Config
    from .cluster.spec import from_flags
    if args.ps_hosts or args.worker_hosts:
        return from_flags(args.ps_hosts or "", args.worker_hosts or "")
    ps, workers = Config(args.config).get_ps_and_worker_hosts()
    return ClusterSpec({"ps": list(ps), "worker": list(workers)})


def run(args):
    import torch

    import distributedtensorflow_amd as dtf
    from . import ops
    from .data import MixedLabels
    from .parallel import (MirroredStrategy, MultiWorkerMirroredStrategy, OneDeviceStrategy,
                           ParameterServerStrategy)
    from .summary import logger
    from .train import (ConfigProto, MonitoredTrainingSession, StopAtStepHook,
                        get_or_create_global_step)

    print("run main with args =", args, flush=True)
    check_data_args(args)
    batch, opt_name, lr = DEFAULTS[args.model]
    batch = args.batch_size or batch
    opt_name = args.optimizer or opt_name
    if opt_name == "adamw":
        lr = 1e-4                      # the BERT paper's; image models must name theirs (main)
    lr = args.learning_rate if args.learning_rate is not None else lr
    if args.clip_norm is not None and args.job_name:
        from .optimizers.base import CLIP_BETWEEN_GRAPH
        raise SystemExit(CLIP_BETWEEN_GRAPH)
    accum = args.accumulation_steps
    if accum < 1:
        raise SystemExit(f"--accumulation_steps {accum} must be at least 1")
    if accum > 1 and args.job_name:
        from .optimizers.base import ACCUM_BETWEEN_GRAPH
        raise SystemExit(ACCUM_BETWEEN_GRAPH)
    if args.ema_decay is not None:
        from .optimizers.moving_averages import EMA_BETWEEN_GRAPH
        if args.job_name:
            raise SystemExit(EMA_BETWEEN_GRAPH)
        if not 0.0 < args.ema_decay < 1.0:
            raise SystemExit(f"--ema_decay {args.ema_decay} outside (0, 1)")
    want_gpu = (args.device == "gpu" or
                (args.device == "auto" and torch.cuda.is_available() and args.num_gpus != 0))

    server = None
    if args.job_name:                                   # ---- between-graph PS cluster
        from .cluster import Server
        cluster = _cluster_from_args(args)
        server = Server(cluster, job_name=args.job_name, task_index=args.task_index)
        if args.job_name == "ps":
            print("Started Parameter Server ...", flush=True)
            stats = server.join()
            print("Close Parameter Server ...", stats, flush=True)
            if not stats.get("interrupted"):
                server.shutdown()
            return 0
        if want_gpu:
            device = torch.device("cuda", args.task_index % torch.cuda.device_count())
        else:
            device = torch.device("cpu")
        strategy = ParameterServerStrategy(server=server, sync=args.sync_replicas,
                                           replicas_to_aggregate=args.replicas_to_aggregate,
                                           variable_placement=args.variable_placement,
                                           device=device)
    else:                                               # ---- tf.distribute strategies
        name = args.strategy or ("mirrored" if want_gpu else "onedevice")
        if name == "onedevice":
            strategy = OneDeviceStrategy("/gpu:0" if want_gpu else "/cpu:0")
        elif name == "mirrored":
            strategy = MirroredStrategy(bucket_mb=args.bucket_mb)
        elif name == "multiworker":
            strategy = MultiWorkerMirroredStrategy(bucket_mb=args.bucket_mb)
        else:
            strategy = ParameterServerStrategy(num_ps=args.num_ps,
                                               variable_placement=args.variable_placement)
        device = strategy.device
    rid, nrep = strategy.replica_id, strategy.num_replicas_in_sync
    is_chief = strategy.is_chief
    torch.manual_seed(args.seed)
    dtype = torch.bfloat16 if device.type == "cuda" else torch.float32

    # ---- data + model
    num_classes = None
    if args.image_data:
        if args.model.startswith("bert"):
            raise SystemExit("--image_data needs an image model")
        num_classes = args.num_classes or (10 if args.model.startswith("mnist") else 1000)
        if args.model == "mnist_mlp" and num_classes != 10:
            raise SystemExit("mnist_mlp has 10 classes")
        shards = nrep if server is None else 1
        data = _image_dataset(args, "train", num_classes, batch, device, dtype, shards,
                              rid if shards > 1 else 0)
        batch = data.batch_size
    elif args.text_data:
        shards = nrep if server is None else 1
        data = _token_dataset(args, "train", batch, device, shards, rid if shards > 1 else 0)
        batch = data.batch_size
    elif args.model.startswith("mnist"):
        from .data import DeviceArrayDataset, mnist
        imgs, labels = mnist.load_arrays(args.data_dir, "train")
        if args.download_only:
            mnist.load_arrays(args.data_dir, "test")
            return 0
        shards = nrep if server is None else 1
        data = DeviceArrayDataset(imgs, labels, batch, device, dtype, shuffle=False,
                                  num_shards=shards, shard_index=rid if shards > 1 else 0)
    elif args.model.startswith("resnet"):
        from .data import SyntheticImageNet
        data = SyntheticImageNet(batch, args.image_size, device=device, dtype=dtype,
                                 seed=1234 + rid)
    else:
        from .data import SyntheticMLM
        data = SyntheticMLM(batch, args.seq_len, device=device, seed=1234 + rid)
        if args.causal_lm:
            _causal_batches(data)

    with strategy.scope():
        if num_classes is not None and args.model != "mnist_mlp":
            ctor = dtf.models.MnistCNN if args.model == "mnist_cnn" else \
                getattr(dtf.models, args.model)
            model = ctor(num_classes=num_classes)
        elif args.model == "mnist_cnn":
            model = dtf.models.MnistCNN()
        elif args.model == "mnist_mlp":
            model = dtf.models.MnistMLP(args.hidden_units)
        elif args.model.startswith("resnet"):
            model = getattr(dtf.models, args.model)()
        elif args.text_data:
            from .models import bert
            model = getattr(bert, args.model)(vocab_size=data.masking.vocab_size,
                                              causal=args.causal_lm)
        else:
            from .models import bert
            model = getattr(bert, args.model)(causal=args.causal_lm)
        model.train()
        global_step = get_or_create_global_step()
        ema = None
        if args.ema_decay is not None:
            ema = dtf.train.ExponentialMovingAverage(args.ema_decay, num_updates=global_step)
        opt = _make_optimizer(opt_name, lr, args.model, batch * nrep * accum, args.max_steps,
                              args.clip_norm, ema, accum)
        if args.sync_replicas and server is not None:
            nw = len(server.worker_ranks())
            opt = dtf.train.SyncReplicasOptimizer(
                opt, replicas_to_aggregate=args.replicas_to_aggregate or nw, total_num_replicas=nw)
        opt.build(list(model.parameters()))

    def micro_step():
        if args.model.startswith("bert"):
            b = next(data)
            w = b.get("masked_lm_weights")
            if w is None:                      # the synthetic set predicts every slot
                w = torch.ones_like(b["masked_lm_ids"], dtype=torch.float32)
            loss = model(b["input_ids"], b["segment_ids"], b["input_mask"],
                         b["masked_lm_positions"], b["masked_lm_ids"], w)
        else:
            x, y = next(data)
            logits = model(x)
            if isinstance(y, MixedLabels):
                loss = ops.mixed_softmax_cross_entropy(logits, *y, args.label_smoothing)
            elif args.model == "mnist_mlp":
                onehot = torch.nn.functional.one_hot(y, 10).to(logits.dtype)
                loss = ops.softmax_cross_entropy_clipped_sum(logits, onehot)
            else:
                loss = ops.sparse_softmax_cross_entropy(logits, y, args.label_smoothing)
        opt.minimize(loss, global_step=global_step)
        return loss

    def train_op():
        # one update per run: hooks, logging and --train_steps count updates
        if accum == 1:
            return {"loss": micro_step()}
        losses = [micro_step().detach().float() for _ in range(accum)]
        return {"loss": torch.stack(losses).mean()}

    # ---- evaluation: every replica of a strategy evaluates its shard; in a between-graph
    # cluster the chief worker alone does, on the variables it pulled
    eval_fn = eval_hook = None
    if (args.eval or args.eval_every) and (server is None or is_chief):
        eval_fn = _make_eval_fn(args, model, opt, strategy, device, dtype, batch,
                                nrep if server is None else 1, rid if server is None else 0,
                                ema)
    hooks = [StopAtStepHook(last_step=args.max_steps)]
    if eval_fn is not None and args.eval_every:
        from .train import EvalHook
        eval_hook = EvalHook(eval_fn, args.eval_every)
        hooks.append(eval_hook)
    cfg = ConfigProto(allow_soft_placement=True, intra_op_parallelism_threads=os.cpu_count(),
                      inter_op_parallelism_threads=os.cpu_count())
    logs = None
    t0, first_step, last = time.time(), None, None
    with MonitoredTrainingSession(master=server.target if server else "", is_chief=is_chief,
                                  checkpoint_dir=args.checkpoint_dir, config=cfg, hooks=hooks,
                                  model=model, optimizer=opt, global_step=global_step,
                                  strategy=strategy, save_checkpoint_steps=args.save_checkpoint_steps,
                                  save_checkpoint_secs=args.save_checkpoint_secs,
                                  log_step_count_steps=None, save_summaries_steps=None) as sess:
        if is_chief and args.log_dir:
            stamp = datetime.datetime.now().strftime("%Y_%m_%d__%H_%M_%S")
            log_directory = os.path.join(args.log_dir, stamp)
            logs = logger.TensorBoardOutputFormat(dir=log_directory)
            print("Logging to", log_directory, flush=True)
            if eval_hook is not None:
                eval_hook.writer = logs
        first_step = global_step.value()
        while not sess.should_stop():
            out = sess.run([train_op, "loss", global_step])
            if out is None:
                break
            _, loss, gstep = out
            last = (loss, gstep)
            if is_chief and args.log_every and gstep % args.log_every == 0:
                print("Worker ({}): loss = {:0.2f} (global step: {})".format(
                    args.task_index if server else rid, loss, gstep), flush=True)
                if logs is not None:
                    logs.writekvs({"Global Step": gstep, "Loss": loss}, global_step=gstep)
    if device.type == "cuda":
        torch.cuda.synchronize()
    elapsed = time.time() - t0
    if logs is not None:
        logs.close()
    result = {"model": args.model, "strategy": type(strategy).__name__, "replicas": nrep,
              "global_step": global_step.value(), "elapsed_s": round(elapsed, 2),
              "final_loss": None if last is None else round(float(last[0]), 4)}
    if args.clip_norm is not None and last is not None:
        # the last step's pre-clip norm: the one host read of it
        result["grad_norm"] = round(float(opt.last_grad_norm.item()), 6)
    if accum > 1:
        result["accumulation_steps"] = accum
    for k in ("mixup_alpha", "cutmix_alpha"):
        if getattr(args, k):
            result[k] = getattr(args, k)
    if args.randaugment:
        for k in ("randaugment", "ra_magnitude", "ra_mstd", "ra_prob"):
            result[k] = getattr(args, k)
    if args.whole_word_mask:
        result["whole_word_mask"] = True
    if args.causal_lm:
        result["causal_lm"] = True
    steps_done = global_step.value() - (first_step or 0)
    if steps_done > 0 and server is None:
        result["examples_per_sec"] = round(steps_done * batch * nrep * accum / elapsed, 1)
    ev = None
    if eval_fn is not None and args.eval:
        ev = eval_fn()                     # collective: every replica of the strategy is here
    elif eval_hook is not None and eval_hook.results:
        ev = eval_hook.results[-1][1]
    if ev is not None:
        result["eval_loss"] = round(ev["loss"], 4)
        result["eval_top_1"] = round(ev["top_1"], 4)
        result["eval_top_k"] = round(ev["top_k"], 4)
        for k in ("ema_loss", "ema_top_1", "ema_top_k"):
            if k in ev:
                result["eval_" + k] = round(ev[k], 4)
        if args.causal_lm:
            # The perplexity is exp of the eval_loss printed next to it, i.e. of the loss rounded
            # to 4 places, so that the two reported figures agree exactly.  eval_top_1 is the
            # next-token accuracy and eval_count the number of predicted (non-pad) next tokens.
            result["eval_perplexity"] = math.exp(result["eval_loss"])
        if args.image_data or args.text_data or args.causal_lm:
            result["eval_count"] = int(ev["count"])
        elif args.model.startswith("mnist"):
            result["test_accuracy"] = round(ev["top_1"], 4)
    if is_chief:
        print(json.dumps(result), flush=True)
    if server is not None:
        server.shutdown()
    return 0


def _image_dataset(args, split, num_classes, batch, device, dtype, shards, shard_index):
    """--image_data: the HBM-resident ``split`` of DIR as a DeviceImageDataset.  ResNets get
    --image_size outputs under the ImageNet channel statistics, the MNIST models 28 x 28 x 1
    scaled to [0, 1]; the batch shrinks to the shard where that is smaller."""
    from .data import DeviceImageDataset, ImageAugment, ImageMix, ImageRandAugment, images
    from .data.images import IMAGENET_MEAN, IMAGENET_STD
    imgs, labels = images.load_arrays(args.image_data, split, num_classes)
    C = imgs.shape[3]
    if args.model.startswith("mnist"):
        if C != 1:
            raise SystemExit(f"{args.model} takes 1-channel images; {args.image_data} has {C}")
        size, mean, std = 28, None, None
    else:
        if C != 3:
            raise SystemExit(f"{args.model} takes 3-channel images; {args.image_data} has {C}")
        size, mean, std = args.image_size, IMAGENET_MEAN, IMAGENET_STD
    mode = {"rrc": "random_resized_crop", "pad_crop": "pad_crop", "none": "none"}[args.augment]
    aug = ImageAugment(size, mode=mode, mean=mean, std=std)
    batch = max(1, min(batch, len(range(shard_index, len(labels), shards))))
    # between-graph workers all hold the whole set: each shuffles and augments on its own stream
    stream = args.task_index if args.job_name else shard_index
    mix = None
    if split == "train" and (args.mixup_alpha or args.cutmix_alpha):
        mix = ImageMix(args.mixup_alpha, args.cutmix_alpha)
    rand = None
    if split == "train" and args.randaugment:
        rand = ImageRandAugment(args.randaugment, args.ra_magnitude, args.ra_mstd, args.ra_prob)
    return DeviceImageDataset(imgs, labels, batch, device, aug, dtype=dtype,
                              shuffle=split == "train", seed=args.seed + stream,
                              aug_seed=args.seed + 1000003 * (stream + 1),
                              num_shards=shards, shard_index=shard_index,
                              flatten=args.model == "mnist_mlp", mix=mix,
                              mix_seed=args.seed + 2000003 * (stream + 1), rand=rand,
                              rand_seed=args.seed + 3000017 * (stream + 1))


def _causal_batches(data):
    """--causal_lm without --text_data: the SyntheticMLM pool's ``input_ids`` / ``input_mask``
    as next-token batches (``causal_lm_targets``), in place."""
    from .data import causal_lm_targets
    for i, b in enumerate(data.batches):
        labels, weights = causal_lm_targets(b["input_ids"], b["input_mask"])
        data.batches[i] = {"input_ids": b["input_ids"], "segment_ids": b["segment_ids"],
                           "input_mask": b["input_mask"], "masked_lm_positions": None,
                           "masked_lm_ids": labels, "masked_lm_weights": weights}
    return data


def _token_dataset(args, split, batch, device, shards, shard_index):
    """--text_data: the HBM-resident ``split`` of DIR as a DeviceTokenDataset under --mlm_prob /
    --max_predictions (and DIR/meta.json, where present), with DIR/continuation.npy under
    --whole_word_mask; the batch shrinks to the shard where that is smaller.  Under --causal_lm
    the rows come out unmasked with next-token targets."""
    from .data import DeviceTokenDataset, TokenMasking, load_continuation, load_token_arrays
    tokens, masking = load_token_arrays(args.text_data, split, TokenMasking(prob=args.mlm_prob))
    continuation = None
    if args.whole_word_mask:
        try:
            continuation = load_continuation(args.text_data, masking)
        except (FileNotFoundError, ValueError) as e:
            raise SystemExit(f"--whole_word_mask: {e}")
    S = tokens.shape[1]
    if args.causal_lm:
        if S > 512:
            raise SystemExit(f"{args.text_data}: rows of {S} tokens; the sequence length is at "
                             "most 512")
    elif S > 512 or args.max_predictions > S:
        raise SystemExit(f"{args.text_data}: rows of {S} tokens; the sequence length is at most "
                         f"512 and at least --max_predictions ({args.max_predictions})")
    if device.type == "cuda" and S % 64:
        raise SystemExit(f"{args.text_data}: rows of {S} tokens; the attention kernel needs a "
                         "sequence length that is a multiple of 64")
    batch = max(1, min(batch, len(range(shard_index, len(tokens), shards))))
    # between-graph workers all hold the whole set: each shuffles and masks on its own stream
    stream = args.task_index if args.job_name else shard_index
    return DeviceTokenDataset(tokens, batch, device, masking, args.max_predictions,
                              shuffle=split == "train", seed=args.seed + stream,
                              mask_seed=args.seed + 1000003 * (stream + 1),
                              eval_seed=args.seed & 0xFFFFFFFF, num_shards=shards,
                              shard_index=shard_index, continuation=continuation,
                              objective="causal" if args.causal_lm else "mlm")


def _make_eval_fn(args, model, opt, strategy, device, dtype, batch, shards, shard_index,
                  ema=None):
    """-> eval_fn() -> {"loss", "top_1", "top_k", "count"}: one pass of this replica's shard of
    the evaluation set through ``train.evaluate`` (collective under a collective strategy).
    With ``ema`` a second pass evaluates the averaged weights: "ema_loss", "ema_top_1",
    "ema_top_k"."""
    from .metrics import ClassificationMetrics
    from .train import evaluate
    if args.image_data:
        num_classes = args.num_classes or (10 if args.model.startswith("mnist") else 1000)
        data = _image_dataset(args, "val", num_classes, batch, device, dtype, shards, shard_index)

        def batches():
            return data.single_pass()
    elif args.text_data:
        data = _token_dataset(args, "val", batch, device, shards, shard_index)

        def batches():
            return data.single_pass()
    elif args.model.startswith("mnist"):
        from .data import DeviceArrayDataset, mnist
        imgs, labels = mnist.load_arrays(args.data_dir, "test")
        per = max(1, min(1000, len(labels) // shards))
        data = DeviceArrayDataset(imgs, labels, per, device, dtype, shuffle=False,
                                  num_shards=shards, shard_index=shard_index)

        def batches():
            return data.single_pass()
    else:
        if args.model.startswith("resnet"):
            from .data import SyntheticImageNet
            data = SyntheticImageNet(batch, args.image_size, device=device, dtype=dtype,
                                     pool=max(1, min(2, args.eval_steps)),
                                     seed=4321 + shard_index)
        else:
            from .data import SyntheticMLM
            data = SyntheticMLM(batch, args.seq_len, device=device, seed=4321 + shard_index,
                                pool=max(1, min(2, args.eval_steps)))
            if args.causal_lm:
                _causal_batches(data)

        def batches():
            return data.single_pass(args.eval_steps)
    metrics = ClassificationMetrics(k=args.eval_top_k, strategy=strategy)

    def eval_fn():
        metrics.reset()
        res = evaluate(model, batches(), metrics, optimizer=opt, strategy=strategy)
        if ema is not None:
            metrics.reset()
            avg = evaluate(model, batches(), metrics, optimizer=opt, strategy=strategy,
                           averages=ema)
            res.update({"ema_" + k: avg[k] for k in ("loss", "top_1", "top_k")})
        return res
    return eval_fn


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    parser = build_parser()
    args, _unparsed = parser.parse_known_args(argv)
    if args.optimizer == "lars" and args.learning_rate is None:
        # no LARS learning rate has been validated on real data: there is no default to fall to
        parser.error("--optimizer lars requires --learning_rate")
    if args.optimizer == "adamw" and args.learning_rate is None and \
            not args.model.startswith("bert"):
        parser.error("--optimizer adamw requires --learning_rate with an image model")
    check_data_args(args)
    if (args.num_gpus or 0) > 1 and "WORLD_SIZE" not in os.environ and not args.job_name:
        return _spawn_local(args, argv)
    return run(args)


if __name__ == "__main__":
    sys.exit(main())
