"""Host side of the evaluation kernels (csrc/evaluate_kernels.hip, the matches-only entry of csrc/sample_kernels.hip): the
reference's quantitative evaluation, ``DenseCorrespondenceEvaluation.evaluate_network``
(dense_correspondence/evaluation/evaluation.py:475-527) and what it calls per image pair
(single_same_scene_image_pair_quantitative_analysis :862-958, compute_descriptor_match_statistics :1007-1178), on the frames
of a ``frames.FrameStore``.

``choose_pairs`` draws the image pairs on the host (a few integers per pair).  ``evaluate_frame_pairs`` then gathers the
frames, normalizes them, runs the network in eval mode, finds and subsamples the ground-truth matches and computes every
column of the reference's table for all pairs, without reading anything back; ``evaluate_network`` composes the two and
copies the table to the host once.

``compute_descriptor_statistics_on_dataset`` (csrc/descstats_kernels.hip) is the first quantitative part of the reference's
``run_evaluation_on_network`` (evaluation.py:2157-2304): the per-channel min, max and mean of the descriptors over random
frames of the store, for the whole image and for the object mask, written to ``descriptor_statistics.yaml``.

``evaluate_network`` above, called on the train and on the test store, is the second part.

``evaluate_network_cross_scene`` (csrc/crossscene_kernels.hip) is the third, ``evaluate_network_cross_scene``
(evaluation.py:253-301, single_cross_scene_image_pair_quantitative_analysis :610-781): the only table built from human-labelled
matches between DIFFERENT scenes.  ``cross_scene_labels`` resolves the annotated pairs to store frames,
``choose_cross_scene_views`` draws the other views of either scene on the host, and ``evaluate_cross_scene_rows`` reprojects the
labelled pixels into them (``reproject_pixels``), runs the network once per distinct frame and computes the table's rows with
every searched image read once (``match_statistics_groups``).

``evaluate_network_cross_instance`` feeds the same chain with every combination of two pixel-labelled images.

``evaluate_network_cross_scene_keypoints`` is the class-consistent keypoint table (evaluation.py:407-472, single_image_pair_
cross_scene_keypoints_quantitative_analysis :1433-1552): named keypoints on different object instances, every combination of two
labelled images, both orders (``keypoint_labels``, ``keypoint_rows``, ``evaluate_keypoint_rows``, ``keypoint_table``).  A labelled
image is searched by (images - 1) * keypoints rows there, which is what ``match_statistics_groups_wide`` (the row-per-lane
kernel of csrc/crossscene_kernels.hip) is for.

``evaluate_network_across_objects`` (csrc/acrossobj_kernels.hip) is its fourth part, ``evaluate_network_across_objects``
(evaluation.py:305-337): pairs of frames of two different objects (``choose_object_pairs``), pixels sampled from mask a and
their best matches over the whole of image b (``evaluate_object_pairs``: ``across_object_queries`` + ``best_match_pairs``).

``evaluate_network_qualitative`` (csrc/picture_kernels.hip) is the qualitative part, ``evaluate_network_qualitative``
(evaluation.py:1979-2070): per image pair the descriptor pictures of ``plot_descriptor_colormaps`` (``descriptor_pictures`` over
``normalize_descriptor``, ``normalize_descriptor_pair``, ``normalize_masked_descriptor_pair``), sampled pixels with their best
matches, and the distance heat maps of the heat-map tool (``heat_maps``) -- the arithmetic only, nothing OpenCV draws.

One module per table -- pairs, across_objects, cross_scene, keypoints, descstats, curves, pictures -- over the steps they share (_chain);
every name is also reachable as ``dcn_hip.evaluate.<name>``.
"""
from .. import augment as _aug  # noqa: F401
from ._chain import (BAD_DRAWS, BAD_FRAME, BAD_INDEX, BAD_OFFSETS, COLUMNS, TOO_FEW_MASK_PIXELS, EvalTable,  # noqa: F401
                     _forward_in_eval_mode, _gather_frame_list, _gather_host_frames)
from .pairs import (NUM_ATTEMPTS, EvalMatches, choose_pairs, evaluate_frame_pairs, evaluate_network,  # noqa: F401
                    find_eval_matches, match_statistics_pairs)
from .across_objects import (ACROSS_OBJECT_COLUMNS, AcrossObjectTable, AcrossQueries, BestMatches,  # noqa: F401
                             across_object_queries, best_match_pairs, choose_object_pairs, evaluate_network_across_objects,
                             evaluate_object_pairs)
from .cross_scene import (LABELLED, VIEW_OF_A, VIEW_OF_B, CrossSceneLabels, Reprojection,  # noqa: F401
                          choose_cross_scene_views, cross_scene_labels, cross_scene_table, evaluate_cross_scene_rows,
                          evaluate_network_cross_instance, evaluate_network_cross_scene, match_statistics_groups,
                          match_statistics_groups_wide, reproject_pixels)
from .keypoints import (KEYPOINT_COLUMNS, KEYPOINT_ROW_COLUMNS, REVERSE, STANDARD, WIDE_GROUP_MIN_ROWS,  # noqa: F401
                        KeypointLabels, evaluate_keypoint_rows, evaluate_network_cross_scene_keypoints, keypoint_labels,
                        keypoint_rows, keypoint_table)
from .descstats import (STAT_FIELDS, STAT_SETS, choose_frames, combine_descriptor_statistics,  # noqa: F401
                        compute_descriptor_statistics_on_dataset, descriptor_statistics)
from .curves import (CURVE_DROP_NAN, CURVE_EMPTY, CURVE_FIELDS, CURVE_NAN, CURVE_NONFINITE, CURVE_SUMMARY,  # noqa: F401
                     MAX_CURVE_BINS, MAX_CURVES, EvalCurves, area_above_curve, cumulative_frequencies, curves_to_host,
                     evaluation_curves, write_stats_yaml)
from .pictures import (EMPTY_RANGE, HEATMAP_KERNEL_VARIANCE, QUALITATIVE_COLUMNS, DescriptorPictures, HeatMaps,  # noqa: F401
                       Normalized, QualitativeResult, Ranges, choose_qualitative_pairs, colour_table, descriptor_pictures,
                       descriptor_ranges, evaluate_network_qualitative, heat_maps, normalize_descriptor,
                       normalize_descriptor_pair, normalize_masked_descriptor_pair, pictures_to_host, save_qualitative)
