"""CLI mirror of the reference's src/train_rec.py:17-93 for the in-scope models (BPRMF, VBPR, GradFashion, ACF, AttentiveFashion).

Same flag names and defaults for every flag BPRMF/VBPR consume; new flags: --optimizer, --dtype, --init_seed, and GradFashion's
--embed_color / --embed_edges, which the reference reads (GradFashion.py:28-29) but never defines: they default to 20, the
--embed_d default.  ACF's --layers_component / --layers_item are `type=list` in the reference (only the default [64, 1] is
reachable there); here they take two ints `h 1`, and so does AttentiveFashion's --attention_layers.  --dropout is the rate of the
three encoders' Dropout layers (the reference's constant 0.5).
--af_new_users PATH (attentive_fashion only) fits rows for users the model was not trained on and writes new-user-recs-* files.
--acf_new_users PATH (acf only) does the same for ACF: each row is fitted through both attention levels over the user's history.
--similar_items K (bprmf, vbpr, grad_fashion) writes sim-* / best-sim-* files with every item's K nearest items by cosine in the
space of --similar_space (latent: Gi; visual: f E; both), and with --new_items new-sim-* / best-new-sim-* (the visual space).
--diversify THETA (bprmf, vbpr, grad_fashion) writes div-recs-* / div-ild-* files next to recs-*: every user's top_k picked by
greedy Maximal Marginal Relevance from the user's top --diversify_pool, cosines in the space of --similar_space.
--because L (bprmf, vbpr, grad_fashion) writes because-* / best-because-* files next to recs-*: for every recommended (u, i) the L
items of u's training list nearest to i by cosine in the space of --similar_space ("because it is like the X you own"), and with
--new_users / --new_items because-new-user-recs-* / because-new-recs-*.
--influence L (bprmf, vbpr, grad_fashion) writes influence-* / best-influence-* files next to recs-*: for every recommended (u, i) the
L entries of u's training list the score rests on most, by influence on u's own fold-in objective (include/bprx.h, bprx_influence),
and with --new_users influence-new-user-recs-*.
--audience K (bprmf, vbpr, grad_fashion) writes audience-* / best-audience-* files next to recs-*: for every catalogue item (or
the ids of --audience_items) the K users that score it highest, its owners excluded, and with --new_items new-audience-* /
best-new-audience-* (the visual score of items the model was not trained on).
--af_new_items EDGES COLOUR CLASSES, --af_warm_items PATH and --af_audience K (attentive_fashion only) are the warm-item and
audience products of AttentiveFashion: Gi rows for new items from their first buyers (warm-recs-*, warm-audience-*) and
audience-* for the catalogue, each row with its three attentions.
--item_classes PATH with --shelves K / --class_cap M (bprmf, vbpr, grad_fashion) writes shelf-recs-* (every user's K best items of
every item class, the classes in the user's order) and cap-recs-* (the top_k with at most M items of any class) next to recs-*, and
with --new_users shelf-new-user-recs-* / cap-new-user-recs-*.
--styles S [--style_iters T] [--style_top R] (bprmf, vbpr, grad_fashion) clusters the item space of --similar_space into S styles
(spherical k-means) and writes styles-*, style-items-* and user-styles-* next to recs-*, with --new_items also new-styles-*;
--item_classes styles makes the styles the classes of --shelves / --class_cap.
--calibrate LAMBDA with --item_classes (bprmf, vbpr, grad_fashion) writes cal-recs-* / cal-kl-* files next to recs-*: every user's
top_k picked from the user's top --calibrate_pool so that the list's class mix follows the mix of the user's training items
(greedy KL re-rank, include/bprx.h, bprx_calibrate), and with --new_users cal-new-user-recs-* / cal-new-user-kl-*.
--warm_items PATH (bprmf, vbpr, grad_fashion) fits Gi / Bi rows for new items from their first buyers (rows `row<TAB>user`; vbpr and
grad_fashion: rows of the --new_items table) and writes warm-recs-* / best-warm-recs-* files, with --audience K also warm-audience-*.
Run as `python -m fashionvisualexpl_recommend_amd.train_rec --rec bprmf --dataset <name> ...`.
"""
import argparse
import os

from . import configs

CALIBRATE_CLASSES_MAX = 1024                                  # classes --calibrate takes (bprx_calibrate's limit)

_last_model = None


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description="Run train of the Recommender Model.")
    parser.add_argument('--gpu', type=int, default=0, help='HIP device ordinal (the reference default -1 = CPU has '
                                                            'no counterpart: this engine is GPU-only)')
    parser.add_argument('--best_metric', type=str, default='ndcg')
    parser.add_argument('--dataset', nargs='?', default='amazon_baby', help='dataset name')
    parser.add_argument('--rec', nargs='?', default="vbpr", help="bprmf | vbpr | grad_fashion | acf | attentive_fashion")
    parser.add_argument('--batch_size', type=int, default=256, help='batch_size')
    parser.add_argument('--top_k', type=int, default=20, help='top-k of recommendation.')
    parser.add_argument('--epochs', type=int, default=200, help='Number of epochs.')
    parser.add_argument('--verbose', type=int, default=-1, help='number of epochs to store model parameters.')
    parser.add_argument('--batch_eval', type=int, default=128, help='batch size on items for evaluation.')
    parser.add_argument('--lr', type=float, default=0.001, help='Learning rate.')
    parser.add_argument('--validation', type=bool, default=True, help='True to use validation set, False otherwise')
    parser.add_argument('--restore_epochs', type=int, default=1)
    parser.add_argument('--list_of_regs', nargs='+', type=float, default=[0.0], help='list of regularization terms')
    parser.add_argument('--cnn_model', nargs='?', default='vgg19', help='Model used for feature extraction.')
    parser.add_argument('--output_layer', nargs='?', default='fc2', help='Output layer for feature extraction.')
    parser.add_argument('--embed_k', type=int, default=128, help='Embedding size.')
    parser.add_argument('--embed_d', type=int, default=20, help='size of low dimensionality for visual features')
    parser.add_argument('--reg', type=float, default=0, help='regularization')
    # read by GradFashion.py:28-29, defined nowhere in the reference: the --embed_d default
    parser.add_argument('--embed_color', type=int, default=20, help='grad_fashion: size of the colour embedding (Ec columns)')
    parser.add_argument('--embed_edges', type=int, default=20, help='grad_fashion: size of the edge embedding (Ee columns)')
    parser.add_argument('--layers_component', nargs='+', type=int, default=[64, 1],
                        help='acf: component-level attention layers, two ints "h 1" (ACF.py:40)')
    parser.add_argument('--layers_item', nargs='+', type=int, default=[64, 1],
                        help='acf: item-level attention layers, two ints "a 1" (ACF.py:41)')
    parser.add_argument('--acf_gradient', default='detached', choices=['detached', 'full'],
                        help="acf: 'detached' = the reference's step (g'_u is a constant of the tape, ACF.py:203-208); 'full' = the "
                             "same loss differentiated through both attention levels")
    parser.add_argument('--acf_explain', type=int, default=0,
                        help="acf: also write expl-* / best-expl-* files with the L (1..32) history entries that contribute most to "
                             "every recommended (u, i): alpha, contribution and the peak of the component attention; 0 = off")
    parser.add_argument('--attention_layers', nargs='+', type=int, default=[64, 1],
                        help='attentive_fashion: attention layers, two ints "h 1" (train_rec.py:38)')
    parser.add_argument('--af_explain', type=int, default=0,
                        help="attentive_fashion: also write expl-* / best-expl-* files with the exact split of every recommended "
                             "(u, i) score over colour, edges and class and the edges share over a G x G grid of the edge image "
                             "(G = 1, 2, 4, 7, 8, 14 or 16); 0 = off")
    parser.add_argument('--feat_explain', type=int, default=0,
                        help="vbpr, grad_fashion: also write expl-* / best-expl-* files with the L (1..32) feature columns that "
                             "contribute most to every written (u, i): column and contribution F_ic w_uc, rank 0 first; 0 = off")
    parser.add_argument('--new_items', nargs='+', default=None, metavar='PATH',
                        help="vbpr: one .npy of raw feature rows [n, D]; grad_fashion: two, colour then edges.  Items the model was "
                             "not trained on: also write new-recs-* / best-new-recs-* files with every user's top-k of them by the "
                             "visual score Tu.(fE) + f.Bp (rows divided by the training max-abs), and with --feat_explain L also "
                             "new-expl-* / best-new-expl-*")
    parser.add_argument('--new_users', default=None, metavar='PATH',
                        help="bprmf, vbpr, grad_fashion: a TSV of `label<TAB>item` rows, the histories of users the model was not "
                             "trained on (labels are free text, kept in first-appearance order).  Their rows are fitted with the "
                             "item side frozen and new-user-recs-* / best-new-user-recs-* files (label, item, score) are written "
                             "next to recs-* / best-recs-*")
    parser.add_argument('--af_new_users', default=None, metavar='PATH',
                        help="attentive_fashion: a TSV in the format of --new_users.  Each new user's row of Gu is fitted with the "
                             "item side, the encoders and the attention frozen and dropout off, and new-user-recs-* / "
                             "best-new-user-recs-* files (label, item, score, alpha_colour, alpha_edges, alpha_class) are written "
                             "next to recs-* / best-recs-*")
    parser.add_argument('--acf_new_users', default=None, metavar='PATH',
                        help="acf: a TSV in the format of --new_users.  Each new user's row of Gu is fitted by the full derivative "
                             "of the user's own loss through both attention levels over the user's history, everything else "
                             "frozen, and new-user-recs-* / best-new-user-recs-* files (label, item, score) are written next to "
                             "recs-* / best-recs-*")
    parser.add_argument('--similar_items', type=int, default=0, metavar='K',
                        help="bprmf, vbpr, grad_fashion: also write sim-* / best-sim-* files next to recs-* / best-recs-* with every "
                             "catalogue item's K (1..1024) nearest items by cosine in the model's item space, rows `i j cosine`, "
                             "the item itself excluded; with --new_items also new-sim-* / best-new-sim-*, the catalogue neighbours "
                             "of every new item, rows `j_new i cosine`, always in the visual space; 0 = off")
    parser.add_argument('--similar_space', default=None, choices=['latent', 'visual', 'both'],
                        help="--similar_items: latent = Gi, visual = f E (vbpr, grad_fashion; fp32 or bf16 features), both = "
                             "[Gi | f E]; default: latent for bprmf, visual for vbpr and grad_fashion")
    parser.add_argument('--diversify', type=float, default=0.0, metavar='THETA',
                        help="bprmf, vbpr, grad_fashion: also write div-recs-* / best-div-recs-* files next to recs-* / best-recs-* "
                             "with every user's top_k picked by greedy Maximal Marginal Relevance from the user's top "
                             "--diversify_pool: each pick maximises (1 - THETA) relevance - THETA (largest cosine with the picks "
                             "above it), cosines in the space of --similar_space; rows `u i score redundancy` in list order, and "
                             "div-ild-* / best-div-ild-* with one row `u ild` per user (1 - mean pairwise cosine of the list); "
                             "with --new_users also div-new-user-recs-* / div-new-user-ild-*.  THETA in [0, 1]; 0 = off")
    parser.add_argument('--diversify_pool', type=int, default=100, metavar='N',
                        help="--diversify: candidates per user the lists are picked from, top_k <= N <= 1024")
    parser.add_argument('--calibrate', type=float, default=0.0, metavar='LAMBDA',
                        help="bprmf, vbpr, grad_fashion, with --item_classes: also write cal-recs-* / best-cal-recs-* files next to "
                             "recs-* / best-recs-* with every user's top_k picked from the user's top --calibrate_pool so that the "
                             "list's class mix follows the mix of the user's training items (Steck 2018): each pick maximises "
                             "(1 - LAMBDA) relevance - LAMBDA (the change of KL(history mix || list mix) it makes); rows `u i score "
                             "class gain` in list order, and cal-kl-* / best-cal-kl-* with one row `u kl_plain kl_calibrated "
                             "hist_classed` per user; with --new_users also cal-new-user-recs-* / cal-new-user-kl-*.  LAMBDA in "
                             "[0, 1]; 0 = off")
    parser.add_argument('--calibrate_pool', type=int, default=100, metavar='N',
                        help="--calibrate: candidates per user the lists are picked from, top_k <= N <= 1024")
    parser.add_argument('--calibrate_alpha', type=float, default=0.01, metavar='ALPHA',
                        help="--calibrate: the list's class mix is smoothed to (1 - ALPHA) list + ALPHA history; in (0, 1)")
    parser.add_argument('--because', type=int, default=0, metavar='L',
                        help="bprmf, vbpr, grad_fashion: also write because-* / best-because-* files next to recs-* / best-recs-*: "
                             "for every (u, i) of every user's top_k list the L (1..32) items of u's training list nearest to i by "
                             "cosine in the space of --similar_space, rows `u i score rank hist_item cosine`, rank 0 first (a pair "
                             "without an owned item to compare with: one row with rank -1); with --new_users also "
                             "because-new-user-recs-* (the history is the file's), with --new_items also because-new-recs-* "
                             "(always the visual space); 0 = off")
    parser.add_argument('--influence', type=int, default=0, metavar='L',
                        help="bprmf, vbpr, grad_fashion: also write influence-* / best-influence-* files next to recs-* / best-recs-*: "
                             "for every (u, i) of every user's top_k list the L (1..32) entries of u's training list the score rests "
                             "on most -- how far it would fall, to first order, had u not bought the entry (one damped Newton step on "
                             "u's own fold-in objective over --fold_negatives sampled negatives per entry, seed --init_seed) -- rows "
                             "`u i score rank hist_item influence share`, rank 0 first, share = influence / sum of |influence| over "
                             "all of u's entries (a pair without entries: one row with rank -1); with --new_users also "
                             "influence-new-user-recs-* (the fitted rows and the pairs that fitted them); 0 = off")
    parser.add_argument('--influence_damp', type=float, default=1.0, metavar='DAMP',
                        help="--influence: the ridge added to the Hessian A of u's objective is 2 reg pairs + DAMP trace(A) / (k + d); "
                             "DAMP > 0 bounds its condition number by (k + d) / DAMP + 1; 0 needs --reg > 0")
    parser.add_argument('--audience', type=int, default=0, metavar='K',
                        help="bprmf, vbpr, grad_fashion: also write audience-* / best-audience-* files next to recs-* / best-recs-* "
                             "with the K (1..1024) users that score every catalogue item highest, the item's owners (the users "
                             "whose training list names it) excluded, rows `i u score`, item by item, best first; with --new_items "
                             "also new-audience-* / best-new-audience-*, the audience of every new item by the visual score, rows "
                             "`j_new u score`; 0 = off")
    parser.add_argument('--audience_items', default=None, metavar='PATH',
                        help="--audience: a text file with one catalogue item id per line, the items whose audience is written "
                             "(default: the whole catalogue)")
    parser.add_argument('--warm_items', default=None, metavar='PATH',
                        help="bprmf, vbpr, grad_fashion: a TSV of `row<TAB>user` rows, the first buyers (catalogue users) of items the "
                             "model was not trained on; vbpr, grad_fashion: `row` is a row of the --new_items table (required), bprmf: "
                             "the file defines max row + 1 items.  Each item's Gi / Bi row is fitted with everything else frozen "
                             "(the item as the positive against sampled negatives of its buyers, and as often as the negative of "
                             "other users' items) and warm-recs-* / best-warm-recs-* files (u, row, score: every user's top_k warm "
                             "items, bought ones excluded) are written next to recs-* / best-recs-*; with --audience K also "
                             "warm-audience-* / best-warm-audience-* (row, u, score).  A row without buyers keeps zero Gi / Bi and "
                             "scores as in new-recs-*")
    parser.add_argument('--item_classes', default=None, metavar='PATH',
                        help="bprmf, vbpr, grad_fashion: the class (category) of every catalogue item, a TSV of `item<TAB>class` rows "
                             "with non-negative integer class ids, every item exactly once; or the literal `dataset`: the argmax of "
                             "every item's original/features/one_hot_encodings/{i}.npy.  Read by --shelves and --class_cap; "
                             "or the literal `styles`: the clusters of --styles, made from the model that writes the files")
    parser.add_argument('--shelves', type=int, default=0, metavar='K',
                        help="bprmf, vbpr, grad_fashion: also write shelf-recs-* / best-shelf-recs-* files next to recs-* / "
                             "best-recs-*: every user's K (1..1024) best items of every class of --item_classes, training items "
                             "excluded, rows `u class i score`, the user's classes ordered by their best item's score, each shelf "
                             "best first; with --new_users also shelf-new-user-recs-*; 0 = off")
    parser.add_argument('--shelf_count', type=int, default=0, metavar='S',
                        help="--shelves: only every user's first S shelves; 0 = all")
    parser.add_argument('--class_cap', type=int, default=0, metavar='M',
                        help="bprmf, vbpr, grad_fashion: also write cap-recs-* / best-cap-recs-* files next to recs-* / best-recs-*: "
                             "every user's top_k with at most M items of any one class of --item_classes, rows `u i score class`, "
                             "best first; with --new_users also cap-new-user-recs-*; 0 = off")
    parser.add_argument('--styles', type=int, default=0, metavar='S',
                        help="bprmf, vbpr, grad_fashion: cluster the item space of --similar_space into S (2..1024) styles by "
                             "spherical k-means and write styles-* (rows `i style cosine`, every item, -1 for a zero row), "
                             "style-items-* (rows `style size rank i cosine`, every style's --style_top members nearest its "
                             "centroid) and user-styles-* (rows `u style owned share`, the styles of every user's training list) "
                             "next to recs-* / best-recs-*; with --new_items also new-styles-* (rows `j_new style cosine`, visual "
                             "space); `--item_classes styles` makes the styles the classes of --shelves / --class_cap; 0 = off")
    parser.add_argument('--style_iters', type=int, default=20, metavar='T',
                        help="--styles: Lloyd iterations at the most (the loop stops when no item changes its style)")
    parser.add_argument('--style_top', type=int, default=10, metavar='R',
                        help="--styles: members per style in style-items-* (1..1024)")
    parser.add_argument('--af_new_items', nargs=3, default=None, metavar=('EDGES.npy', 'COLOUR.npy', 'CLASSES.npy'),
                        help="attentive_fashion: the inputs of n items the model was not trained on: edge images uint8 [n, 224, 224], "
                             "raw colour histograms [n, Dc] (each divided by its own max-abs, as the catalogue's are; an all-zero "
                             "histogram is rejected) and class vectors [n, Dk]; read by --af_warm_items")
    parser.add_argument('--af_warm_items', default=None, metavar='PATH',
                        help="attentive_fashion: a TSV of `row<TAB>user` rows in the format of --warm_items, the first buyers "
                             "(catalogue users) of the rows of the --af_new_items tables (required).  The score is linear in an "
                             "item's Gi row, so each new item's row is fitted with everything else frozen and dropout off (the item "
                             "as the positive against sampled negatives of its buyers, and as often as the negative of other "
                             "users' items) and warm-recs-* / best-warm-recs-* files (u, row, score, alpha_colour, alpha_edges, "
                             "alpha_class: every user's top_k warm items, bought ones excluded) are written next to recs-* / "
                             "best-recs-*; with --af_audience K also warm-audience-* / best-warm-audience-* (row, u, score, alpha...; "
                             "the item's buyers excluded).  A row without buyers keeps a zero Gi row and scores 0.0 for everyone")
    parser.add_argument('--af_audience', type=int, default=0, metavar='K',
                        help="attentive_fashion: also write audience-* / best-audience-* files next to recs-* / best-recs-* with the K "
                             "(1..1024) users that score every catalogue item highest, the item's owners excluded, rows `i u score "
                             "alpha_colour alpha_edges alpha_class`, item by item, best first; with --af_warm_items also "
                             "warm-audience-* / best-warm-audience-*; 0 = off")
    parser.add_argument('--fold_steps', type=int, default=30,
                        help='--new_users / --af_new_users / --acf_new_users / --warm_items / --af_warm_items: optimiser steps per new '
                             'user or item')
    parser.add_argument('--fold_negatives', type=int, default=4,
                        help='--new_users / --af_new_users / --acf_new_users: sampled negatives per history item; --warm_items / '
                             '--af_warm_items: per buyer')
    # not in the reference
    parser.add_argument('--dropout', type=float, default=0.5,
                        help="attentive_fashion: rate of the encoders' Dropout layers (AttentiveFashion.py:53,62,70: 0.5)")
    parser.add_argument('--optimizer', default='adam_tf23', choices=['adam_tf23', 'sgd'])
    parser.add_argument('--dtype', default='fp32', choices=['fp32', 'bf16', 'fp8'],
                        help='storage type of the feature table F (fp8 = OCP e4m3fn codes of f*448)')
    parser.add_argument('--init_seed', type=int, default=0)
    parser.add_argument('--world_size', type=int, default=1,
                        help='> 1: one process per GPU under torch.distributed.run (reads RANK / WORLD_SIZE / LOCAL_RANK)')
    parser.add_argument('--shard', default='item', choices=['item', 'user'],
                        help='item: VBPR, items + features range-partitioned, users replicated; user: BPRMF, users partitioned')
    parser.add_argument('--sampler', default='ref_stream', choices=['ref_stream', 'philox'],
                        help="ref_stream: the reference's MT19937 index stream (single GPU); philox: device epoch walk "
                             "(always used with --world_size > 1: negatives stay GPU-local)")
    parser.add_argument('--hard_negatives', type=int, default=0,
                        help="C in 2..16: every negative is the best-scored of C sampled candidates under the current model "
                             "(dynamic negative sampling; bprmf, vbpr, grad_fashion with --sampler philox on one GPU); 0 = off. "
                             "File names then end in -hard_C")
    parser.add_argument('--hard_refresh', type=int, default=0,
                        help="with --hard_negatives: take the snapshot of the item projections the candidates are scored with "
                             "again every N steps inside an epoch (it is always taken at an epoch's start); 0 = only there")
    parser.add_argument('--dense_reduce', default='gather', choices=['gather', 'allreduce'],
                        help='multi-GPU VBPR: how the gradient of E / beta-prime is summed over the ranks (dist.py)')
    parser.add_argument('--dist_backend', default='nccl', choices=['nccl', 'gloo'], help='nccl == RCCL on ROCm')
    parser.add_argument('--data_root', default=None, help="overrides the reference's '../data'")
    parser.add_argument('--results_root', default=None, help="overrides the reference's '../results'")
    args = parser.parse_args(argv)
    for name in ("layers_component", "layers_item", "attention_layers"):
        v = getattr(args, name)
        if len(v) != 2 or v[1] != 1 or v[0] <= 0:
            parser.error("--%s takes two ints 'h 1' with h > 0 (got %s)" % (name, " ".join(str(x) for x in v)))
    if args.acf_gradient != 'detached' and args.rec != 'acf':
        parser.error("--acf_gradient %s needs --rec acf (got --rec %s)" % (args.acf_gradient, args.rec))
    if not 0 <= args.acf_explain <= 32:
        parser.error("--acf_explain takes 0 (off) .. 32 (got %s)" % args.acf_explain)
    if args.acf_explain != 0 and args.rec != 'acf':
        parser.error("--acf_explain %s needs --rec acf (got --rec %s)" % (args.acf_explain, args.rec))
    if args.af_explain not in (0, 1, 2, 4, 7, 8, 14, 16):
        parser.error("--af_explain takes 0 (off), 1, 2, 4, 7, 8, 14 or 16 (got %s)" % args.af_explain)
    if args.af_explain != 0 and args.rec != 'attentive_fashion':
        parser.error("--af_explain %s needs --rec attentive_fashion (got --rec %s)" % (args.af_explain, args.rec))
    if not 0 <= args.feat_explain <= 32:
        parser.error("--feat_explain takes 0 (off) .. 32 (got %s)" % args.feat_explain)
    if args.feat_explain != 0 and args.rec not in ('vbpr', 'grad_fashion'):
        parser.error("--feat_explain %s needs --rec vbpr or grad_fashion (got --rec %s)" % (args.feat_explain, args.rec))
    if args.new_items is not None:
        want = {'vbpr': 1, 'grad_fashion': 2}.get(args.rec)
        if want is None:
            parser.error("--new_items needs --rec vbpr or grad_fashion (got --rec %s)" % args.rec)
        if len(args.new_items) != want:
            parser.error("--new_items takes %d path%s with --rec %s (got %d)" % (want, "s" if want > 1 else "", args.rec,
                                                                                 len(args.new_items)))
    if args.new_users is not None and args.rec not in ('bprmf', 'vbpr', 'grad_fashion'):
        parser.error("--new_users needs --rec bprmf, vbpr or grad_fashion (got --rec %s)" % args.rec)
    if args.af_new_users is not None and args.rec != 'attentive_fashion':
        parser.error("--af_new_users needs --rec attentive_fashion (got --rec %s)" % args.rec)
    if args.acf_new_users is not None and args.rec != 'acf':
        parser.error("--acf_new_users needs --rec acf (got --rec %s)" % args.rec)
    if args.warm_items is not None:
        if args.rec not in ('bprmf', 'vbpr', 'grad_fashion'):
            parser.error("--warm_items needs --rec bprmf, vbpr or grad_fashion (got --rec %s)" % args.rec)
        if args.rec != 'bprmf' and args.new_items is None:
            parser.error("--warm_items needs --new_items with --rec %s (the rows of the file are rows of that table)" % args.rec)
        try:
            read_warm_items(args.warm_items)
        except (OSError, ValueError) as e:
            parser.error("--warm_items: %s" % e)
    if args.af_new_items is not None and args.rec != 'attentive_fashion':
        parser.error("--af_new_items needs --rec attentive_fashion (got --rec %s)" % args.rec)
    if args.af_warm_items is not None:
        if args.rec != 'attentive_fashion':
            parser.error("--af_warm_items needs --rec attentive_fashion (got --rec %s)" % args.rec)
        if args.af_new_items is None:
            parser.error("--af_warm_items needs --af_new_items (the rows of the file are rows of those tables)")
        try:
            read_warm_items(args.af_warm_items)
        except (OSError, ValueError) as e:
            parser.error("--af_warm_items: %s" % e)
    if not 0 <= args.af_audience <= 1024:
        parser.error("--af_audience takes 0 (off) .. 1024 (got %s)" % args.af_audience)
    if args.af_audience != 0 and args.rec != 'attentive_fashion':
        parser.error("--af_audience needs --rec attentive_fashion (got --rec %s)" % args.rec)
    if args.fold_steps < 1 or args.fold_negatives < 1:
        parser.error("--fold_steps and --fold_negatives take values >= 1 (got %s, %s)" % (args.fold_steps, args.fold_negatives))
    if not 0 <= args.similar_items <= 1024:
        parser.error("--similar_items takes 0 (off) .. 1024 (got %s)" % args.similar_items)
    if not 0.0 <= args.diversify <= 1.0:                      # (NaN fails both comparisons)
        parser.error("--diversify takes theta in [0, 1], 0 = off (got %s)" % args.diversify)
    if args.diversify > 0 and not args.top_k <= args.diversify_pool <= 1024:
        parser.error("--diversify_pool takes top_k (%d) .. 1024 (got %s)" % (args.top_k, args.diversify_pool))
    if not 0 <= args.because <= 32:
        parser.error("--because takes 0 (off) .. 32 (got %s)" % args.because)
    if not 0 <= args.influence <= 32:
        parser.error("--influence takes 0 (off) .. 32 (got %s)" % args.influence)
    if not (args.influence_damp >= 0 and args.influence_damp < float("inf")):
        parser.error("--influence_damp takes a finite value >= 0 (got %s)" % args.influence_damp)
    if args.influence != 0 and args.rec not in ('bprmf', 'vbpr', 'grad_fashion'):
        parser.error("--influence needs --rec bprmf, vbpr or grad_fashion (got --rec %s)" % args.rec)
    if args.influence != 0 and args.influence_damp == 0 and not args.reg > 0:
        parser.error("--influence_damp 0 needs --reg > 0: without either the Hessian of a user's objective may be singular")
    if args.styles != 0 and not 2 <= args.styles <= 1024:
        parser.error("--styles takes 0 (off) or 2 .. 1024 (got %s)" % args.styles)
    if args.style_iters < 1:
        parser.error("--style_iters takes T >= 1 (got %s)" % args.style_iters)
    if not 1 <= args.style_top <= 1024:
        parser.error("--style_top takes 1 .. 1024 (got %s)" % args.style_top)
    if args.styles == 0 and (args.style_iters != 20 or args.style_top != 10):
        parser.error("--style_iters / --style_top need --styles S")
    if args.item_classes == 'styles' and args.styles == 0:
        parser.error("--item_classes styles needs --styles S")
    asked = args.similar_items != 0 or args.similar_space is not None or args.diversify > 0 or args.because != 0 or args.styles != 0
    if args.similar_space is None:                            # the model's own space
        args.similar_space = {'bprmf': 'latent', 'vbpr': 'visual', 'grad_fashion': 'visual'}.get(args.rec)
    if asked:
        if args.rec not in ('bprmf', 'vbpr', 'grad_fashion'):
            parser.error("--similar_items / --similar_space / --diversify / --because / --styles need --rec bprmf, vbpr or "
                         "grad_fashion (got --rec %s)" % args.rec)
        if args.similar_space != 'latent' and args.rec == 'bprmf':
            parser.error("--similar_space %s needs --rec vbpr or grad_fashion (bprmf has the latent space only)" % args.similar_space)
        if args.similar_space != 'latent' and args.dtype == 'fp8':
            parser.error("--similar_space %s runs with --dtype fp32 or bf16 (got fp8): use --similar_space latent" % args.similar_space)
    if args.styles != 0 and args.new_items is not None and args.similar_space != 'visual':
        parser.error("--styles with --new_items writes new-styles-* in the visual space: --similar_space %s does not go with "
                     "--new_items here" % args.similar_space)
    if not 0 <= args.audience <= 1024:
        parser.error("--audience takes 0 (off) .. 1024 (got %s)" % args.audience)
    if args.audience != 0 and args.rec not in ('bprmf', 'vbpr', 'grad_fashion'):
        parser.error("--audience needs --rec bprmf, vbpr or grad_fashion (got --rec %s)" % args.rec)
    if args.audience_items is not None:
        if args.audience == 0:
            parser.error("--audience_items needs --audience K")
        try:
            read_audience_items(args.audience_items)
        except (OSError, ValueError) as e:
            parser.error("--audience_items: %s" % e)
    if not 0 <= args.shelves <= 1024:
        parser.error("--shelves takes 0 (off) .. 1024 (got %s)" % args.shelves)
    if args.shelf_count < 0:
        parser.error("--shelf_count takes S >= 0, 0 = all (got %s)" % args.shelf_count)
    if args.shelf_count != 0 and args.shelves == 0:
        parser.error("--shelf_count needs --shelves K")
    if args.class_cap < 0:
        parser.error("--class_cap takes M >= 1, 0 = off (got %s)" % args.class_cap)
    if not 0.0 <= args.calibrate <= 1.0:                      # (NaN fails both comparisons)
        parser.error("--calibrate takes lambda in [0, 1], 0 = off (got %s)" % args.calibrate)
    if args.calibrate > 0 and not args.top_k <= args.calibrate_pool <= 1024:
        parser.error("--calibrate_pool takes top_k (%d) .. 1024 (got %s)" % (args.top_k, args.calibrate_pool))
    if not 0.0 < args.calibrate_alpha < 1.0:
        parser.error("--calibrate_alpha takes alpha in (0, 1) (got %s)" % args.calibrate_alpha)
    if args.calibrate > 0 and args.rec not in ('bprmf', 'vbpr', 'grad_fashion'):
        parser.error("--calibrate needs --rec bprmf, vbpr or grad_fashion (got --rec %s)" % args.rec)
    if args.calibrate > 0 and args.item_classes is None:
        parser.error("--calibrate needs --item_classes PATH (or --item_classes dataset / styles)")
    if args.shelves != 0 or args.class_cap != 0 or args.item_classes is not None:
        if args.rec not in ('bprmf', 'vbpr', 'grad_fashion'):
            parser.error("--item_classes / --shelves / --class_cap need --rec bprmf, vbpr or grad_fashion (got --rec %s)" % args.rec)
        if args.item_classes is None:
            parser.error("--shelves / --class_cap need --item_classes PATH (or --item_classes dataset)")
        if args.item_classes not in ('dataset', 'styles'):
            try:
                table = read_item_classes(args.item_classes)
            except (OSError, ValueError) as e:
                parser.error("--item_classes: %s" % e)
            if args.calibrate > 0 and table.size and int(table.max()) + 1 > CALIBRATE_CLASSES_MAX:
                parser.error("--calibrate takes at most %d classes (--item_classes has %d)"
                             % (CALIBRATE_CLASSES_MAX, int(table.max()) + 1))
    if args.hard_negatives != 0 and not 2 <= args.hard_negatives <= 16:
        parser.error("--hard_negatives takes 0 (off) or 2 .. 16 (got %s)" % args.hard_negatives)
    if args.hard_negatives != 0 and args.sampler != 'philox':
        parser.error("--hard_negatives needs --sampler philox (got --sampler %s)" % args.sampler)
    if args.hard_negatives != 0 and args.rec not in ('bprmf', 'vbpr', 'grad_fashion'):
        parser.error("--hard_negatives needs --rec bprmf, vbpr or grad_fashion (got --rec %s)" % args.rec)
    if args.hard_negatives != 0 and int(args.world_size) != 1:
        parser.error("--hard_negatives runs on one GPU (got --world_size %s)" % args.world_size)
    if args.hard_refresh < 0:
        parser.error("--hard_refresh takes N >= 0 (got %s)" % args.hard_refresh)
    if args.hard_refresh != 0 and args.hard_negatives == 0:
        parser.error("--hard_refresh needs --hard_negatives C")
    if not 0.0 <= args.dropout < 1.0:
        parser.error("--dropout takes a rate in [0, 1) (got %s)" % args.dropout)
    return args


def read_audience_items(path, num_items=None):
    """The --audience_items file: one catalogue item id per line -> the ids in file order (repeats kept).  Empty lines are
    skipped; a line that is no integer, a negative id and (with num_items) an id outside the catalogue raise ValueError with the
    line's number."""
    ids = []
    with open(path) as f:
        for ln, line in enumerate(f, 1):
            if not line.strip():
                continue
            try:
                i = int(line.strip())
            except ValueError:
                raise ValueError("%s:%d: the item %r is not an integer" % (path, ln, line.strip())) from None
            if i < 0 or (num_items is not None and i >= num_items):
                raise ValueError("%s:%d: the audience item %d is outside the catalogue%s" % (
                    path, ln, i, "" if num_items is None else " [0, %d)" % num_items))
            ids.append(i)
    return ids


def check_audience_items(args, num_items):
    """--audience_items against the loaded catalogue: an id outside it ends the run as a rejected argument does (parse_args knows
    no catalogue; it has rejected everything else)."""
    if getattr(args, "audience_items", None) is None:
        return
    try:
        read_audience_items(args.audience_items, num_items)
    except ValueError as e:
        argparse.ArgumentParser(description="Run train of the Recommender Model.").error("--audience_items: %s" % e)


def read_item_classes(path, num_items=None):
    """The --item_classes file: rows `item<TAB>class`, two non-negative integers -> the class of every item, an int64 array indexed
    by item ([num_items]; without num_items: [largest item + 1], -1 where the file has no line).  Empty lines are skipped; a line
    that is not two non-negative integers, a repeated item and (with num_items) an item outside the catalogue raise ValueError with
    the line's number; with num_items an item without a line raises ValueError naming the item."""
    import numpy as np
    seen = {}
    with open(path) as f:
        for ln, line in enumerate(f, 1):
            line = line.rstrip("\r\n")
            if not line.strip():
                continue
            parts = line.split("\t")
            try:
                if len(parts) != 2:
                    raise ValueError
                item, cls = int(parts[0]), int(parts[1])
            except ValueError:
                raise ValueError("%s:%d: expected `item<TAB>class`, two integers, got %r" % (path, ln, line)) from None
            if item < 0 or cls < 0:
                raise ValueError("%s:%d: item and class are not negative, got %r" % (path, ln, line))
            if num_items is not None and item >= num_items:
                raise ValueError("%s:%d: the item %d is outside the catalogue [0, %d)" % (path, ln, item, num_items))
            if item in seen:
                raise ValueError("%s:%d: the item %d has a class already (line %d)" % (path, ln, item, seen[item][0]))
            seen[item] = (ln, cls)
    out = np.full(max(seen, default=-1) + 1 if num_items is None else num_items, -1, np.int64)
    for item, (_, cls) in seen.items():
        out[item] = cls
    if num_items is not None and (out < 0).any():
        raise ValueError("%s: the item %d has no class (every catalogue item appears exactly once)" % (path, int(np.flatnonzero(out < 0)[0])))
    return out


def dataset_item_classes(dataset, num_items):
    """--item_classes dataset: the argmax of every item's one-hot class vector original/features/one_hot_encodings/{i}.npy (the
    table AttentiveFashion reads whole) -> int64 [num_items].  A missing file raises ValueError naming it."""
    import numpy as np
    d = configs.class_features_path_dir(dataset)
    out = np.empty(num_items, np.int64)
    for i in range(num_items):
        f = d + "%d.npy" % i
        if not os.path.exists(f):
            raise ValueError("--item_classes dataset: the class vector %s is missing" % f)
        out[i] = int(np.argmax(np.asarray(np.load(f)).reshape(-1)))
    return out


def check_item_classes(args, num_items):
    """--item_classes against the loaded catalogue, before anything is trained: an item outside it or without a class (or a missing
    class vector of the dataset) ends the run as a rejected argument does.  Returns the table, int64 [num_items] (None without the
    flag; an array that is there already is returned as it is), so that it is read once per run."""
    src = getattr(args, "item_classes", None)
    if src is None or not isinstance(src, str) or src == 'styles':     # (the styles are made by the model that stores)
        return src
    try:
        return dataset_item_classes(args.dataset, num_items) if src == 'dataset' else read_item_classes(src, num_items)
    except (OSError, ValueError) as e:
        argparse.ArgumentParser(description="Run train of the Recommender Model.").error("--item_classes: %s" % e)


def read_warm_items(path, num_rows=None):
    """The --warm_items file: rows `row<TAB>user` -> one list of buyers per new item, buyers[row] in file order (repeats kept).
    num_rows: the rows of the --new_items table the file refers to (None: the file defines max row + 1 items); rows without a
    line have no buyers.  Empty lines are skipped; a line that is not two integers, a negative row or user and a row past the
    table raise ValueError with the line's number."""
    pairs = []
    with open(path) as f:
        for ln, line in enumerate(f, 1):
            line = line.rstrip("\r\n")
            if not line.strip():
                continue
            parts = line.split("\t")
            try:
                if len(parts) != 2:
                    raise ValueError
                row, user = int(parts[0]), int(parts[1])
            except ValueError:
                raise ValueError("%s:%d: expected `row<TAB>user`, two integers, got %r" % (path, ln, line)) from None
            if row < 0 or user < 0:
                raise ValueError("%s:%d: row and user are not negative, got %r" % (path, ln, line))
            if num_rows is not None and row >= num_rows:
                raise ValueError("%s:%d: row %d is past the table of %d new items" % (path, ln, row, num_rows))
            pairs.append((row, user))
    buyers = [[] for _ in range(max((r for r, _ in pairs), default=-1) + 1 if num_rows is None else num_rows)]
    for row, user in pairs:
        buyers[row].append(user)
    return buyers


def read_af_new_items(paths):
    """The --af_new_items tables (edges, colour, classes .npy) -> the three arrays, checked: edges uint8 [n, 224, 224], colour and
    classes real-valued [n, D] with the same n, no colour histogram all zero (its max-abs normalisation would divide by zero).
    ValueError names the file; the widths are checked against the model's Dc, Dk by AttentiveFashion.prepare_new_items."""
    import numpy as np
    if len(paths) != 3:
        raise ValueError("three paths (edges, colour, classes), got %d" % len(paths))
    ed, col, cl = (np.load(p, mmap_mode='r') for p in paths)
    if ed.dtype != np.uint8 or ed.ndim != 3 or ed.shape[1:] != (224, 224):
        raise ValueError("%s: edges must be uint8 [n, 224, 224], got %s %s" % (paths[0], ed.dtype, ed.shape))
    n = ed.shape[0]
    for p, a, what in ((paths[1], col, "colour"), (paths[2], cl, "classes")):
        if a.ndim != 2 or a.shape[0] != n or a.shape[1] < 1 or a.dtype.kind not in "fiu":
            raise ValueError("%s: %s must be a real-valued [%d, D] table, got %s %s" % (p, what, n, a.dtype, a.shape))
    mx = np.max(np.abs(np.asarray(col)), axis=1) if n else np.zeros(0)
    if not np.all(mx > 0):
        raise ValueError("%s: the colour histogram of row %d is all zero: its max-abs normalisation divides by zero"
                         % (paths[1], int(np.flatnonzero(~(mx > 0))[0])))
    return np.asarray(ed), np.asarray(col), np.asarray(cl)


def read_new_users(path):
    """The --new_users file: rows `label<TAB>item` -> (labels in first-appearance order, one item list per label, in file order).
    Empty lines are skipped; anything else that is not a label and an integer item raises ValueError with its line number."""
    labels, index, lists = [], {}, []
    with open(path) as f:
        for ln, line in enumerate(f, 1):
            line = line.rstrip("\r\n")
            if not line.strip():
                continue
            parts = line.split("\t")
            if len(parts) != 2 or parts[0] == "":
                raise ValueError("%s:%d: expected `label<TAB>item`, got %r" % (path, ln, line))
            try:
                item = int(parts[1])
            except ValueError:
                raise ValueError("%s:%d: the item %r is not an integer" % (path, ln, parts[1])) from None
            if parts[0] not in index:
                index[parts[0]] = len(labels)
                labels.append(parts[0])
                lists.append([])
            lists[index[parts[0]]].append(item)
    return labels, lists


def train(argv=None):
    args = parse_args(argv)
    if args.rec == 'grad_fashion' and int(args.world_size) > 1:
        raise NotImplementedError('--rec grad_fashion runs on one GPU (no multi-GPU form): use --world_size 1')
    if args.feat_explain != 0 and int(args.world_size) > 1:
        raise NotImplementedError('--feat_explain runs on one GPU (the sharded drivers write no expl-* files): use --world_size 1')
    if args.new_items is not None and int(args.world_size) > 1:
        raise NotImplementedError('--new_items runs on one GPU (the sharded drivers write no new-recs-* files): use --world_size 1')
    if args.new_users is not None and int(args.world_size) > 1:
        raise NotImplementedError('--new_users runs on one GPU (the sharded drivers write no new-user-recs-* files): use --world_size 1')
    if args.af_new_users is not None and int(args.world_size) > 1:
        raise NotImplementedError('--af_new_users runs on one GPU (no multi-GPU form): use --world_size 1')
    if args.similar_items != 0 and int(args.world_size) > 1:
        raise NotImplementedError('--similar_items runs on one GPU (the sharded drivers write no sim-* files): use --world_size 1')
    if args.diversify > 0 and int(args.world_size) > 1:
        raise NotImplementedError('--diversify runs on one GPU (the sharded drivers write no div-* files): use --world_size 1')
    if args.calibrate > 0 and int(args.world_size) > 1:
        raise NotImplementedError('--calibrate runs on one GPU (the sharded drivers write no cal-* files): use --world_size 1')
    if args.calibrate > 0 and args.top_k > 1024:
        raise ValueError('--calibrate ranks on the device only (top_k <= 1024): there is no host form')
    if args.because != 0 and int(args.world_size) > 1:
        raise NotImplementedError('--because runs on one GPU (the sharded drivers write no because-* files): use --world_size 1')
    if args.influence != 0 and int(args.world_size) > 1:
        raise NotImplementedError('--influence runs on one GPU (the sharded drivers write no influence-* files): use --world_size 1')
    if args.influence != 0 and args.top_k > 1024:
        raise ValueError('--influence runs on the device only (top_k <= 1024): there is no host form')
    if args.audience != 0 and int(args.world_size) > 1:
        raise NotImplementedError('--audience runs on one GPU (the sharded drivers write no audience-* files): use --world_size 1')
    if args.warm_items is not None and int(args.world_size) > 1:
        raise NotImplementedError('--warm_items runs on one GPU (the sharded drivers write no warm-* files): use --world_size 1')
    if (args.shelves != 0 or args.class_cap != 0) and int(args.world_size) > 1:
        raise NotImplementedError('--shelves / --class_cap run on one GPU (the sharded drivers write no shelf-* / cap-* files): use '
                                  '--world_size 1')
    if args.styles != 0 and int(args.world_size) > 1:
        raise NotImplementedError('--styles runs on one GPU (the sharded drivers write no styles-* files): use --world_size 1')
    if args.class_cap != 0 and min(args.class_cap, args.top_k) > 1024:
        raise ValueError('--class_cap ranks on the device only (min(class_cap, top_k) <= 1024): there is no host form')
    if args.warm_items is not None and args.new_items is not None:                  # a row past the table: before anything is trained
        import numpy as np
        read_warm_items(args.warm_items, int(np.load(args.new_items[0], mmap_mode='r').shape[0]))
    for flag in ("af_new_items", "af_warm_items", "af_audience"):
        if getattr(args, flag) and int(args.world_size) > 1:
            raise NotImplementedError('--%s runs on one GPU (no multi-GPU form): use --world_size 1' % flag)
    if args.af_new_items is not None:                                               # before anything is loaded or trained
        n_new = int(read_af_new_items(args.af_new_items)[0].shape[0])
        if args.af_warm_items is not None:
            read_warm_items(args.af_warm_items, n_new)
    if args.because != 0 and args.top_k > 1024:
        raise ValueError('--because runs on the device only (top_k <= 1024): there is no host form')
    if args.new_items is not None and args.dtype == 'fp8':
        raise ValueError('--new_items runs with --dtype fp32 or bf16 (an fp8 table is scaled for the training max-abs: a new row '
                         'may saturate)')
    if args.rec == 'acf' and int(args.world_size) > 1:
        raise NotImplementedError('--rec acf runs on one GPU (no multi-GPU form): use --world_size 1')
    if args.rec == 'acf' and args.dtype not in ('fp32', 'bf16'):
        raise ValueError('--rec acf runs with --dtype fp32 or bf16 (got %s)' % args.dtype)
    if args.rec == 'attentive_fashion' and int(args.world_size) > 1:
        raise NotImplementedError('--rec attentive_fashion runs on one GPU (no multi-GPU form): use --world_size 1')
    if args.rec == 'attentive_fashion' and args.dtype != 'fp32':
        raise ValueError('--rec attentive_fashion runs with --dtype fp32 (got %s)' % args.dtype)
    configs.set_roots(args.data_root, args.results_root)
    import torch
    from .dataset import DataLoader
    from .models import ACF, BPRMF, VBPR, AttentiveFashion, GradFashion
    os.makedirs(os.path.join(configs.results_dir(), args.dataset, args.rec), exist_ok=True)     # train_rec.py:52-55
    os.makedirs(os.path.join(configs.weight_dir(), args.dataset, args.rec), exist_ok=True)
    world = int(args.world_size)
    if world > 1:                                                                               # one process per GPU
        import torch.distributed as dist
        if int(os.environ.get("WORLD_SIZE", "1")) != world:
            raise SystemExit("--world_size %d needs `python -m torch.distributed.run --nproc-per-node %d ...`" % (world, world))
        args.gpu = int(os.environ.get("LOCAL_RANK", "0")) if os.environ.get("BPRX_ONE_GPU") != "1" else 0
        torch.cuda.set_device(args.gpu)
        if not dist.is_initialized():
            dist.init_process_group(backend=args.dist_backend)
    torch.cuda.set_device(args.gpu)                                                             # train_rec.py:57
    out = []
    for it, current_reg in enumerate(list(args.list_of_regs)):                                  # train_rec.py:60
        print('--------------------------------------------------------------------')
        print('ITERATION %d/%d WITH REGULARIZATION: %f' % (it + 1, len(list(args.list_of_regs)), current_reg))
        data = DataLoader(params=args)
        check_audience_items(args, data.num_items)
        class_table = check_item_classes(args, data.num_items)
        if args.calibrate > 0 and not isinstance(class_table, str) and int(class_table.max()) + 1 > CALIBRATE_CLASSES_MAX:
            raise ValueError('--calibrate takes at most %d classes (--item_classes has %d)'
                             % (CALIBRATE_CLASSES_MAX, int(class_table.max()) + 1))
        if args.warm_items is not None and any(u >= data.num_users for who in read_warm_items(args.warm_items) for u in who):
            raise ValueError('--warm_items: a buyer is outside the %d users of the dataset' % data.num_users)
        if args.af_warm_items is not None and any(u >= data.num_users for who in read_warm_items(args.af_warm_items) for u in who):
            raise ValueError('--af_warm_items: a buyer is outside the %d users of the dataset' % data.num_users)
        print("Training {0} on {1}".format(args.rec, args.dataset))
        print("Parameters:")
        args.reg = current_reg                                                                  # train_rec.py:69
        for arg in vars(args):
            print("\t- " + str(arg) + " = " + str(getattr(args, arg)))
        print("\n")
        args.item_classes = class_table                            # (the table itself from here on: the model does not read it again)
        if world > 1 and args.rec == 'vbpr' and args.shard == 'item':
            from .sharded import ShardedVBPR
            model = ShardedVBPR(data, args)
        elif world > 1 and args.rec == 'bprmf' and args.shard == 'user':
            from .sharded import ShardedBPRMF
            model = ShardedBPRMF(data, args)
        elif world > 1:
            raise NotImplementedError('--world_size > 1 from this CLI: --rec vbpr --shard item, or --rec bprmf --shard user')
        elif args.rec == 'bprmf':
            model = BPRMF(data, args)
        elif args.rec == 'vbpr':
            model = VBPR(data, args)
        elif args.rec == 'grad_fashion':
            model = GradFashion(data, args)
        elif args.rec == 'acf':
            model = ACF(data, args)
        elif args.rec == 'attentive_fashion':
            model = AttentiveFashion(data, args)
        else:
            raise NotImplementedError('Not implemented or unknown Recommender Model.')        # train_rec.py:86
        out.append(model.train())
        global _last_model
        _last_model = model                                        # (tests / interactive use)
        print('END REGULARIZATION')
        print('--------------------------------------------------------------------')
    return out


if __name__ == '__main__':
    train()
