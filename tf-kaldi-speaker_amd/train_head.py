"""Train a new classifier head on a pre-trained, frozen encoder (head_train.py): stage one of
egs/voxceleb/v1/nnet/lib/finetune.py, with its positional arguments.

    python -m tf_kaldi_speaker_amd.train_head [--gpu N] [--checkpoint C] [--config new.json] [--seed S] [--precision P]
                                              [--keep-head] [--segment-layers] [--frame-layers] [--conv-layers] [--batch-norm {moving,batch}] pretrain_model train_dir train_spklist valid_dir valid_spklist
                                              finetune_model

`--config` names the configuration of the NEW model (loss_func, margins, optimizer, learning-rate schedule, batch shape); without
it the pre-trained model's config.json is used.  The network hyper-parameters must be those of the pre-trained model: its
variables are copied unchanged.  `--checkpoint` is a checkpoint name under <pretrain_model>/nnet (default: the one its
`checkpoint` file names).  `--segment-layers` trains the two dense layers behind the pooling node together with the head
(tail_train.py); `--frame-layers` (which implies `--segment-layers`) also trains the 1-tap frame layers between the last
multi-tap convolution and the pooling node, through the gradient of statistics pooling (frame_train.py).  The intended flow is
three runs: the head first, then `--segment-layers --keep-head` on the directory the first run wrote, then
`--frame-layers --keep-head` on the directory of the second.  `--conv-layers` (which implies the other two) trains every
frame-level layer, the multi-tap convolutions included, on the packed features (conv_train.py): a fourth run, on the directory
of the third.  On a `resnet_18` model `--conv-layers` trains every 2-D convolution and residual block, conv5, dense1 and dense2
(resnet_train.py, csrc/gconv_grad.hip); `--frame-layers` alone stays refused there.  `--batch-norm batch` (with any of the three) runs the batch norms of the trained layers in training mode, as
the reference does: the statistics of the batch, the gradient through them, moving-average updates that the checkpoints then
hold (tail_train.batch_stats_options); the default `moving` keeps the moving statistics constant.  On a `self_attention` model
`--frame-layers` and `--conv-layers` also train the key and value networks and the query, through the gradient of the
attentive pooling (att_train.py).  When the configuration's loss_func is `semihard_triplet_loss` or `angular_triplet_loss` the
same switches fine-tune with that loss (metric_losses.MetricHead, csrc/metric_loss_grad.hip): there is no classifier layer, so
one of the three is required, `--keep-head` is accepted and ignored, the checkpoint's own softmax/output/* is copied unchanged,
and the `loss` of an epoch's line is valid.metric_valid's.
One line per epoch: `epoch <e> step <s> loss <valid loss> eer <eer> lr <rate>`."""
import argparse
import os
import sys

from . import model_io
from .params import Params


def build_parser():
    parser = argparse.ArgumentParser(description="Train a new softmax-family head on a frozen pre-trained encoder.")
    parser.add_argument("-g", "--gpu", type=int, default=-1, help="The GPU id (-1: LOCAL_RANK or 0; there is no CPU path).")
    parser.add_argument("--checkpoint", type=str, default="", help="Checkpoint name under <pretrain_model>/nnet (e.g. model-120000); "
                        "default: the one nnet/checkpoint names.")
    parser.add_argument("--config", type=str, default="", help="The configuration file of the new model (default: the pre-trained one).")
    parser.add_argument("--seed", type=int, default=-1, help="Seed of the initialisation and of the batches (default: params.seed or 0).")
    parser.add_argument("--precision", type=str, default="", help="f32 | bf16x3 | f16x3 | f16f6 of the frozen forward (default: the trainer's)")
    parser.add_argument("--keep-head", action="store_true", help="Start from the checkpoint's own softmax kernel when its shape fits.")
    parser.add_argument("--segment-layers", action="store_true", help="Train the two segment-level layers behind the pooling node "
                        "together with the head (everything in front of it stays frozen).")
    parser.add_argument("--frame-layers", action="store_true", help="Also train the 1-tap frame layers behind the last multi-tap "
                        "convolution (tdnn4, tdnn5; tdnn8 .. tdnn10 of the extended TDNN) through the gradient of statistics pooling; "
                        "implies --segment-layers.")
    parser.add_argument("--conv-layers", action="store_true", help="Train every frame-level layer, the multi-tap convolutions "
                        "(tdnn1 .. tdnn3; tdnn1 .. tdnn7 of the extended TDNN) included: nothing stays frozen but the moving "
                        "statistics; implies --frame-layers and --segment-layers.  On a resnet_18 model: every 2-D convolution "
                        "and residual block, conv5, dense1 and dense2 (resnet_train.py).")
    parser.add_argument("--batch-norm", choices=("moving", "batch"), default="moving", help="Batch norm of the trained layers: "
                        "moving = inference mode, the moving statistics stay as the checkpoint has them (default); batch = the "
                        "statistics of the batch, moving-average updates with params.batchnorm_momentum; needs --segment-layers, "
                        "--frame-layers or --conv-layers (the head has no batch norm).")
    parser.add_argument("--verbose", action="store_true", help="One line per step.")
    parser.add_argument("pretrain_model", type=str, help="The pre-trained model directory.")
    parser.add_argument("train_dir", type=str, help="The data directory of the training set.")
    parser.add_argument("train_spklist", type=str, help="The spklist file maps the TRAINING speakers to the indices.")
    parser.add_argument("valid_dir", type=str, help="The data directory of the validation set.")
    parser.add_argument("valid_spklist", type=str, help="The spklist maps the VALID speakers to the indices.")
    parser.add_argument("finetune_model", type=str, help="The fine-tuned model directory")
    return parser


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    from . import head_train
    if args.batch_norm == "batch" and not (args.segment_layers or args.frame_layers or args.conv_layers):
        parser.error(head_train.BATCH_NORM_ALONE)
    nnet_dir = os.path.join(args.pretrain_model, "nnet")
    config_json = args.config or os.path.join(nnet_dir, "config.json")
    if not os.path.isfile(config_json):
        sys.exit("Cannot find params.json in %s" % config_json)
    params = Params(config_json)
    if params.dict.get("loss_func") in ("semihard_triplet_loss", "angular_triplet_loss") and not (
            args.segment_layers or args.frame_layers or args.conv_layers):
        parser.error(head_train.METRIC_HEAD_ONLY % params.dict.get("loss_func"))
    with open(os.path.join(nnet_dir, "feature_dim"), "r") as f:
        dim = int(f.readline().strip())
    if "selected_dim" in params.dict:
        dim = params.selected_dim
    weights, _ = model_io.load_weights(nnet_dir, name=args.checkpoint or None)
    if weights is None:
        sys.exit("[ERROR] Cannot find checkpoint in %s." % nnet_dir)
    from .trainer import Trainer
    trainer = Trainer(params, args.pretrain_model, dim, single_cpu=True, device=args.gpu if args.gpu >= 0 else None,
                      precision=args.precision or None)
    trainer.build("predict")
    trainer.load_weights(weights, 0)
    seed = args.seed if args.seed >= 0 else int(params.dict.get("seed", 0))
    history = head_train.train_head(trainer, args.train_dir, args.train_spklist, args.valid_dir, args.valid_spklist,
                                    args.finetune_model, weights=weights, seed=seed, keep_head=args.keep_head,
                                    precision=args.precision or None, log=print if args.verbose else None,
                                    segment_layers=args.segment_layers or args.frame_layers or args.conv_layers,
                                    frame_layers=args.frame_layers or args.conv_layers, conv_layers=args.conv_layers,
                                    batch_norm=args.batch_norm)
    for epoch, step, loss, eer, lr in history:
        print("epoch %d step %d loss %f eer %f lr %.8f" % (epoch, step, loss, eer, lr))
    trainer.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
